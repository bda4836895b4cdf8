#!/bin/bash
# MFMA-utilisation counters and the instruction mix of the head kernels (field / neck / rgb / plain heads / weight gradients) over a
# short eager bench run.
# Counters in their own pass with --kernel-trace only.  Usage (gpurun): bash tools/pmc_heads.sh <tag> [bench args]
#   -> gpurun_out/pmc_heads_<tag>/summary.json  (copy to profiles/<tag>_mfma_counters.json)
# PASSES (default "1 2") selects the passes.  Pass 3 asks one question of the head backward kernels: do the matrix pipe and the vector
# instructions of a SIMD overlap (matrix-busy and vector-active cycles against busy cycles; profiles/head_bwd_schedule_ab.json).
# EMER_PMC_LIB=<tag> profiles emernerf_amd/lib/libemernerf_<tag>.so (through tools/ab_bench.py) instead of the in-tree build.
# A pass that fails ends the script: nothing more is started on the device behind it.
TAG=${1:-r03}; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/pmc_heads_$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/pmch /tmp/pmch2 /tmp/pmch3 /tmp/pmch4
PASSES=${PASSES:-1 2}
BENCH="python $R/bench.py"
[ -n "$EMER_PMC_LIB" ] && BENCH="python $R/tools/ab_bench.py $EMER_PMC_LIB" && export EMER_LIBSEL_SAME_ABI=1   # (a build of these sources)
BARGS="--full --eager --no-cpu-baseline --no-extras --no-second-state --no-secondary --no-fp16-state --steps 12 --warmup 4 --init-steps 12"
has_pass() { case " $PASSES " in *" $1 "*) return 0 ;; esac; return 1; }
run_pass() {   # <dir> <log> <counters...>
    local dir=$1 log=$2; shift 2
    timeout -k 10 300 rocprofv3 --pmc "$@" --kernel-trace -d $dir -o p --output-format csv -- $BENCH $BARGS $EXTRA > $OUT/$log 2>&1
    local rc=$?
    echo "rc=$rc" >> $OUT/$log
    if [ $rc -ne 0 ]; then echo "pass $log failed (rc=$rc): stopping"; tail -5 $OUT/$log; exit $rc; fi
}
EXTRA="$*"
if has_pass 1; then run_pass /tmp/pmch pass.log SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE; fi
# second pass (own run): instruction mix -- how many vector / matrix / memory instructions a wave issues per launch
if has_pass 2; then run_pass /tmp/pmch2 pass2.log SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_MFMA; fi
# third pass (own run): the four counters of the overlap question in ONE run, so that they describe the same launches
if has_pass 3; then run_pass /tmp/pmch3 pass3.log SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_MFMA GRBM_GUI_ACTIVE; fi
# fourth pass (own run): where a wave's cycles go -- waiting at s_waitcnt (SQ_WAIT_ANY), waiting to issue (SQ_WAIT_INST_ANY, _LDS), issuing
# (SQ_ACTIVE_INST_ANY), all in quad-cycles like SQ_WAVE_CYCLES; and the cycles in which matrix and vector instructions execute together
if has_pass 4; then run_pass /tmp/pmch4 pass4.log SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_COEXEC_CYCLES SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE; fi
python - "$OUT" <<'PY'
import csv, glob, collections, json, sys
out = sys.argv[1]
agg = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter()
dur = collections.defaultdict(float); nd = collections.Counter()
dirs = ('/tmp/pmch', '/tmp/pmch2', '/tmp/pmch3', '/tmp/pmch4')
for fn in [f for d in dirs for f in glob.glob(d + '/**/*counter_collection.csv', recursive=True)]:
    for r in csv.DictReader(open(fn)):
        k = r['Kernel_Name'].replace('void ', '').replace('emer::', '')
        if not any(t in k for t in ('neck_', 'rgb_', 'rmlp_', 'wgrad_stream', 'mlp_chain', 'linear_fwd', 'field_fwd', 'density_', 'ray_wgrad')): continue
        k = k.split('(')[0][:60]
        agg[k][r['Counter_Name']] += float(r['Counter_Value']); cnt[(k, r['Counter_Name'])] += 1
traces = [f for d in dirs for f in glob.glob(d + '/**/*kernel_trace.csv', recursive=True)]
for fn in traces[:1]:
    for r in csv.DictReader(open(fn)):
        k = r['Kernel_Name'].replace('void ', '').replace('emer::', '').split('(')[0][:60]
        if k in agg:
            dur[k] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3; nd[k] += 1
res = {}
for k, d in agg.items():
    c = {n: v / cnt[(k, n)] for n, v in d.items()}
    us = dur[k] / max(nd[k], 1)
    clock_ghz = c.get('GRBM_GUI_ACTIVE', 0.0) / 8.0 / (us * 1e3) if us else 0.0   # GRBM_GUI_ACTIVE sums the 8 XCDs
    busy = c.get('SQ_VALU_MFMA_BUSY_CYCLES', 0.0)
    simd_cycles = 1024.0 * us * 1e3 * clock_ghz
    c.update({"launches": nd[k], "avg_us_traced": us, "effective_clock_ghz": clock_ghz,
              "mfma_busy_frac": busy / simd_cycles if simd_cycles else None})
    if 'SQ_ACTIVE_INST_VALU' in c and simd_cycles:
        # (the raw counters stay in the record: the overlap question is read from these ratios, whatever unit a counter ticks in)
        c["valu_active_frac"] = c['SQ_ACTIVE_INST_VALU'] / simd_cycles
        c["busy_cu_frac"] = c.get('SQ_BUSY_CU_CYCLES', 0.0) / simd_cycles
        c["valu_active_per_inst"] = c['SQ_ACTIVE_INST_VALU'] / c['SQ_INSTS_VALU'] if c.get('SQ_INSTS_VALU') else None
        c["mfma_busy_per_inst"] = busy / c['SQ_INSTS_MFMA'] if c.get('SQ_INSTS_MFMA') else None
    if c.get('SQ_WAVE_CYCLES'):
        c.update({n.lower()[3:] + "_per_wave_cycle": c[n] / c['SQ_WAVE_CYCLES'] for n in ('SQ_WAIT_ANY', 'SQ_WAIT_INST_ANY', 'SQ_WAIT_INST_LDS', 'SQ_ACTIVE_INST_ANY') if n in c})
    res[k] = c
json.dump({"note": "per launch averages; mfma_busy_frac = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x kernel cycles at the effective clock "
                   "GRBM_GUI_ACTIVE / 8 / duration); SQ_INSTS_VALU_MFMA_MOPS_F32 x 512 = fp32 matrix flops; valu_active_frac and "
                   "busy_cu_frac: SQ_ACTIVE_INST_VALU and SQ_BUSY_CU_CYCLES over the same denominator (pass 3)", "kernels": res},
          open(out + '/summary.json', 'w'), indent=1)
for k, c in sorted(res.items(), key=lambda kv: -kv[1]['avg_us_traced'] * kv[1]['launches'])[:12]:
    print(f"{k:55s} n={c['launches']:4d} {c['avg_us_traced']:8.1f} us  clk {c['effective_clock_ghz']:.2f} GHz  mfma busy {c['mfma_busy_frac'] if c['mfma_busy_frac'] is None else round(c['mfma_busy_frac'], 3)}  "
          f"valu active {round(c['valu_active_frac'], 3) if 'valu_active_frac' in c else None}  mops {c.get('SQ_INSTS_VALU_MFMA_MOPS_F32', 0):.3g}")
PY
