#!/bin/bash
# Everything the round's profiles/ directory is built from, in ONE gpurun call:  bash tools/collect_round.sh <tag>
# (kernel trace + timeline, FETCH / WRITE PMC passes, SQ + MFMA counter passes, the default bench line with its CPU baseline,
# the variant configurations).  Summaries land in $OUT/; copy the ones to be judged into profiles/.
TAG=${1:-r04}
R=$GRAFT_REPO_ROOT
export OUT=${BENCH_OUT:-$R/bench_out}; mkdir -p $OUT
python3 $R/bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err
bash $R/tools/profile_round.sh $TAG
bash $R/tools/pmc_sq.sh $TAG
cd $R
python3 tools/pmc_classes.py $OUT/prof_${TAG}_pmc_fetch_size.txt $OUT/prof_${TAG}_pmc_write_size.txt > $OUT/${TAG}_pmc_per_class.json
python3 tools/sq_summary.py $OUT/pmc_${TAG}_1.txt $OUT/pmc_${TAG}_2.txt > $OUT/${TAG}_sq_counters.txt
python3 tools/mfma_summary.py $OUT/pmc_${TAG}_3.txt $OUT/prof_${TAG}_kernel_trace.txt --json $OUT/${TAG}_mfma_per_class.json > $OUT/${TAG}_mfma_busy.txt
MNAS_BENCH_DETAIL=1 python3 bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench_detail.json 2> $OUT/${TAG}_detail.txt
python3 bench.py --full --h2d --no-cpu-baseline --no-roofline > $OUT/${TAG}_bench_h2d.json 2>/dev/null
python3 bench.py --full --k5 --no-cpu-baseline > $OUT/${TAG}_bench_k5.json 2>/dev/null
python3 bench.py --full --se --no-cpu-baseline > $OUT/${TAG}_bench_se.json 2>/dev/null
for hw in 384x512 512x512 512x384; do
  python3 bench.py --full --hw $hw --batch 64 --no-cpu-baseline --no-roofline > $OUT/${TAG}_bench_${hw}.json 2>/dev/null
done
python3 bench.py --clusters --no-cpu-baseline > $OUT/${TAG}_bench_clusters.json 2>/dev/null
python3 bench.py --full --ccf --no-cpu-baseline > $OUT/${TAG}_bench_ccf.json 2>/dev/null
