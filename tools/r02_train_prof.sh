#!/bin/bash
# kernel-trace of the training step (98 304 rays) + PMC passes for its kernels.  Run through gpurun from the repo root.
export TMPDIR=/tmp
REPO=$(pwd)
OUT=$REPO/gpurun_out/${1:-r02_train}
rm -rf $OUT; mkdir -p $OUT
cd /tmp
ARGS="--steps 6 --warmup 2 --no-cpu-baseline --no-teacher"
rocprofv3 --kernel-trace --stats -d $OUT/kt -o kt --output-format csv -- python $REPO/bench.py --full $ARGS > $OUT/kt.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY -d $OUT/pmc1 -o pmc1 --output-format csv -- python $REPO/bench.py --full $ARGS > $OUT/pmc1.log 2>&1
rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc2 -o pmc2 --output-format csv -- python $REPO/bench.py --full $ARGS > $OUT/pmc2.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc3 -o pmc3 --output-format csv -- python $REPO/bench.py --full $ARGS > $OUT/pmc3.log 2>&1
rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU SQ_INSTS_MFMA -d $OUT/pmc4 -o pmc4 --output-format csv -- python $REPO/bench.py --full $ARGS > $OUT/pmc4.log 2>&1
cd $REPO
python - "$OUT" <<'PY'
import csv, glob, collections, json, sys
out_dir = sys.argv[1]
out = {}
for f in sorted(glob.glob(out_dir + '/pmc*/*counter_collection.csv')):
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        name = r['Kernel_Name'].split('(')[0]
        if name.startswith(('r2l_', 'void r2l_')):
            # the 98 304-ray launches only: grids of >= 512 workgroups for the chains, 256 for the dW kernels
            agg[name + ' grid=' + r.get('Grid_Size', '?')][r['Counter_Name']].append(float(r['Counter_Value']))
    for k, d in agg.items():
        for c, v in d.items():
            out.setdefault(k, {})[c] = sum(v) / len(v)
json.dump(out, open(out_dir + '/pmc_summary.json', 'w'), indent=1)
PY
find $OUT -name "*counter_collection.csv" -delete
find $OUT -name "*kernel_trace.csv" -delete
find $OUT -name "*agent_info.csv" -delete
cut -c1-200 $OUT/kt/kt_kernel_stats.csv | head -30
