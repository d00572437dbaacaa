#!/bin/bash
# the round's measurement session: smoke, then rocprofv3 --stats +
# PMC passes of configurations 4 (headline), 5 (at its own 4096 spp by default: C5SPP), 3 and 2, then the PT_DIAG
# counts (profiles/diag_c<N>.json: what bench.py's executed-work model reads).   usage: TAG=r04a OUT=<log dir> bash tools/gpu_profile_all.sh
# (the PMC passes themselves keep their logs where tools/gpu_pmc_cfg.sh puts them)
TAG=${TAG:-r04a}; C5SPP=${C5SPP:-0}; OUT=${OUT:?"OUT=<directory for the session's logs> required"}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
timeout -k 10 120 python __graft_entry__.py smoke > $OUT/smoke.log 2>&1; echo "smoke exit $?"; tail -1 $OUT/smoke.log
DIAGSO=raytracer.c_amd/csrc/librt_hip_diag.so
# PT_DIAG counts first: bench.py below then finds records stamped with today's source hash
RT_HIP_SHIM_PATH=$DIAGSO timeout -k 10 300 python tools/diag.py 4 128 --json profiles/diag_c4.json > $OUT/diag4_$TAG.log 2>&1; echo "diag 4 exit $?"
RT_HIP_SHIM_PATH=$DIAGSO timeout -k 10 400 python tools/diag.py 5 256 --json profiles/diag_c5.json > $OUT/diag5_$TAG.log 2>&1; echo "diag 5 exit $?"
RT_HIP_SHIM_PATH=$DIAGSO timeout -k 10 300 python tools/diag.py 3 256 --json profiles/diag_c3.json > $OUT/diag3_$TAG.log 2>&1; echo "diag 3 exit $?"
RT_HIP_SHIM_PATH=$DIAGSO timeout -k 10 300 python tools/diag.py 2 64 --json profiles/diag_c2.json > $OUT/diag2_$TAG.log 2>&1; echo "diag 2 exit $?"
RT_HIP_SHIM_PATH=$DIAGSO timeout -k 10 300 python tools/diag.py 1 4 --json profiles/diag_c1.json > $OUT/diag1_$TAG.log 2>&1; echo "diag 1 exit $?"
RT_HIP_SHIM_PATH=$DIAGSO timeout -k 10 300 python tools/diag.py 5 64 > $OUT/diag5_64_$TAG.log 2>&1
rm -rf $OUT/profiles_new; mkdir -p $OUT/profiles_new; cp profiles/diag_c*.json $OUT/profiles_new/ 2>/dev/null
TAG=$TAG CONFIG=4 SPP=0 bash tools/gpu_pmc_cfg.sh 2>&1 | tail -13
TAG=$TAG CONFIG=5 SPP=$C5SPP bash tools/gpu_pmc_cfg.sh 2>&1 | tail -13
TAG=$TAG CONFIG=3 SPP=0 bash tools/gpu_pmc_cfg.sh 2>&1 | tail -13
TAG=$TAG CONFIG=2 SPP=0 bash tools/gpu_pmc_cfg.sh 2>&1 | tail -13
cp profiles/pmc_c*.json profiles/${TAG}_c* $OUT/profiles_new/ 2>/dev/null
# the --full line, now with records that match the sources: parity, frac_executed, PMC keys
( time timeout -k 10 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/bench_full_$TAG.log 2> $OUT/bench_full_$TAG.err ) 2>&1 | grep real
echo "bench exit $?"; tail -1 $OUT/bench_full_$TAG.log | cut -c1-300
cp $OUT/bench_full_$TAG.log $OUT/profiles_new/${TAG}_bench_default.json
for c in 4 5 3 2; do cp $OUT/diag${c}_$TAG.log $OUT/profiles_new/${TAG}_diag_c${c}.txt 2>/dev/null; done
tail -4 $OUT/diag5_$TAG.log
