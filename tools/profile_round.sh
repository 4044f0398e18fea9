#!/bin/bash
# All rocprofv3 evidence of a round in one GPU-box call (run from the repo root through gpurun):
#   bash tools/profile_round.sh r3 <commit>
# Writes gpurun_out/prof_<tag>/: kernel stats of the f32 headline bench, of the fp16 mode and of the bf16 DistilBERT forward;
# PMC FETCH_SIZE of the DOMINANT kernel only (--kernel-include-regex attn_paged_kernel: 6.1 k counter records per pass instead of
# 32.6 k -- both profiler aborts of round 2 came from the tool's per-dispatch records on long runs, profiles/README.md) on the
# eager twin of the headline generation AND under hipGraph replay; PMC MFMA utilisation of the DistilBERT GEMMs.
# Counter passes carry --pmc only (no trace domains): the pool refuses the combination.  One attempt per pass, no retries; stderr kept.
set -o pipefail
TAG=${1:-r4}
export MGEA_COMMIT=${2:-unknown}
OUT=gpurun_out/prof_$TAG
export TMPDIR=/tmp
mkdir -p $OUT
T=/tmp/prof_$TAG; rm -rf $T; mkdir -p $T
stats() { f=$(find $1 -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $2; }
pmc() { f=$(find $1 -name "*counter_collection.csv" | head -1); echo $f; }
step() {  # step <name> <seconds> <cmd...>: a pass that TIMES OUT ends the script (nothing further touches the GPU)
  local name=$1 secs=$2; shift 2
  timeout -k 10 $secs "$@" > $OUT/$name.out 2> $OUT/$name.err; local rc=$?
  echo "$name rc=$rc" | tee -a $OUT/rc.txt
  # a pass that TIMED OUT or was killed (124 / 137) ends the script; a crash of the profiler tool itself (139: its SIGSEGV at start-up under --pmc,
  # seen in rounds 2 and 4, stderr kept) is recorded and the next pass -- a fresh process -- goes on
  [ $rc -lt 124 ] || [ $rc -eq 139 ] || exit 1
  return $rc
}
BENCH1="python3 bench.py --full --steps 1 --warmup 1 --no-cpu --no-extra"
GEN1="python3 bench.py --steps 1 --warmup 0 --no-cpu --no-extra --profile-stride 0"

step bench_under_rocprof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/bench -- $BENCH1 && stats $T/bench $OUT/bench_kernel_stats.csv
grep '^{' $OUT/bench_under_rocprof.out > $OUT/bench_under_rocprof.json
step f16_prof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/f16 -- python3 tools/f16_prof.py both && stats $T/f16 $OUT/f16_kernel_stats.csv
step bert_bf16_prof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/bert -- python3 tools/bert_prof.py bf16 && stats $T/bert $OUT/bert_bf16_kernel_stats.csv
step prefill16_prof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/p16 -- python3 tools/prefill_bench.py f16 && stats $T/p16 $OUT/prefill_f16_kernel_stats.csv

# FETCH_SIZE of the attention kernel only, eager twin of the headline generation
export MGEA_PMC_COMMAND="MGEA_DECODER_NOGRAPH=1 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex attn_paged_kernel --output-format csv -- $GEN1"
MGEA_DECODER_NOGRAPH=1 step pmc_fetch_attn_eager 420 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex attn_paged_kernel --output-format csv -d $T/pmc_eager -- $GEN1
f=$(pmc $T/pmc_eager); [ -n "$f" ] && python3 tools/pmc_traffic.py $f FETCH_SIZE > $OUT/pmc_fetch_size_attn.json
# (round 4, VERDICT r3 #2c) FETCH_SIZE of the skinny GEMMs and of the head, eager twin, in two passes of tools/pmc_skinny.sh.  The FC2 instantiation
# gemm_skinny_kernel<..., 8> is left out: the profiler dies with SIGSEGV inside its interception of that launch (four attempts, stack in
# profiles/r4_pmc_fetch_size_skinny_profiler_crash.err)
step pmc_fetch_skinny 450 bash tools/pmc_skinny.sh $OUT 'gemm_skinny_kernel<.*, 2>' skinny_nch2
step pmc_fetch_head 450 bash tools/pmc_skinny.sh $OUT 'head_balanced_kernel' head
# (round 4, VERDICT r3 #1c / missing #3) the f32 long-prompt prefill [64, 1024]: kernel stats and MFMA-busy of its GEMM and attention kernels
step prefill_f32_prof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/p32 -- python3 tools/prefill_bench.py f32 logits && stats $T/p32 $OUT/prefill_f32_kernel_stats.csv
step pmc_mfma_prefill_f32 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-include-regex "gemm_f32_nt_kernel|attn_dense_kernel" --output-format csv -d $T/pmc_p32 -- python3 tools/prefill_bench.py f32 logits
f=$(pmc $T/pmc_p32); [ -n "$f" ] && python3 tools/pmc_mfma.py $f "" > $OUT/pmc_mfma_util_prefill_f32.json
# (round 4) the packed DistilBERT forward, and the in-process A/Bs of the round's switches
step bert_bf16_packed_prof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/bertp -- python3 tools/bert_prof.py bf16 packed && stats $T/bertp $OUT/bert_bf16_packed_kernel_stats.csv
step bert_packed_ab 300 python3 tools/bert_packed_ab.py
step attn16_pipe_ab 300 python3 tools/attn16_ab.py attn16_pipe 0 1
step prefill16_pages_ab 300 python3 tools/prefill_ab.py decoder_prefill16_pages 0 1
step head_phases 300 python3 tools/head_phases.py
step step_ab_head 300 python3 tools/step_ab.py head_balanced 0 1
step step_ab_one_per_cu 300 python3 tools/step_ab.py skinny_one_per_cu 0 1
step sampler_bench 200 python3 tools/sampler_bench.py
# (round 4) the reference's own serving case, B = 1: kernel stats of one greedy generation (split-context decode attention)
step b1_prof 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/b1 -- python3 tools/b1_prof.py && stats $T/b1 $OUT/b1_kernel_stats.csv
# MFMA utilisation of the DistilBERT GEMMs
step pmc_mfma 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_BF16 --kernel-include-regex gemm_bf16_ph_kernel --output-format csv -d $T/pmc_mfma -- python3 tools/bert_prof.py bf16
f=$(pmc $T/pmc_mfma); [ -n "$f" ] && python3 tools/pmc_mfma.py $f gemm > $OUT/pmc_mfma_util.json
# LAST (nothing follows it): the same FETCH_SIZE pass under hipGraph replay (the run bench.py times): with the filter the tool holds 6.1 k records instead of 32.6 k
export MGEA_PMC_COMMAND="rocprofv3 --pmc FETCH_SIZE --kernel-include-regex attn_paged_kernel --output-format csv -- $GEN1 (decode steps replayed from the hipGraph)"
step pmc_fetch_attn_graph 420 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex attn_paged_kernel --output-format csv -d $T/pmc_graph -- $GEN1
f=$(pmc $T/pmc_graph); [ -n "$f" ] && python3 tools/pmc_traffic.py $f FETCH_SIZE > $OUT/pmc_fetch_size_attn_graph_replay.json
ls -la $OUT; cat $OUT/rc.txt
