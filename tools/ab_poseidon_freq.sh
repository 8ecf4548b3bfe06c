#!/bin/bash
# A/B of the partial rounds of the Poseidon permutation: the split state of VX_POSEIDON_SPLIT_PARTIAL (0) vs the state kept in the
# transform domain of the linear layer (VX_POSEIDON_FREQ_PARTIAL=1, csrc/poseidon_freq.h).
#   build  (no GPU needed; after `make -C 0-kno-vectorx_amd/csrc`): build_ab/poseidon_rate_fq{0,1}, 0-kno-vectorx_amd/libvx_pfq{0,1}.so,
#          the compiler's resource report of the Poseidon kernels (build_ab/pfq{0,1}_resources.txt) and the instruction counts of the
#          permutation kernel's basic blocks (build_ab/pfq{0,1}_blocks.txt, tools/asm_blocks.py)
#   run    (on the GPU) the microbenchmark of both -- cycles per wave of the permutation and of a partial round at 4, 6 and 8 waves per
#          SIMD, and the checksum, which must be equal -- then bench.py alternating between a baseline library (VX_AB_BASE, default the
#          macro-0 build) and the macro-1 build, baseline first, three rounds, fresh processes; output under VX_AB_OUT (default build_ab/out)
set -e
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/0-kno-vectorx_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ "$1" = build ]; then
  mkdir -p $R/build_ab
  for v in 0 1; do
    $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -DVX_POSEIDON_FREQ_PARTIAL=$v -I$R/include -o $R/build_ab/poseidon_rate_fq$v $R/tools/poseidon_rate.hip
    $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -DVX_POSEIDON_FREQ_PARTIAL=$v -I$R/include --cuda-device-only -S -o $R/build_ab/poseidon_rate_fq$v.s $R/tools/poseidon_rate.hip
    python3 $R/tools/asm_blocks.py $R/build_ab/poseidon_rate_fq$v.s _Z6k_permPmj ops > $R/build_ab/pfq${v}_blocks.txt
    : > $R/build_ab/pfq${v}_resources.txt
    for f in vx_poseidon vx_fri; do
      $HIPCC -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wno-unused-value -Wno-pass-failed -DVX_POSEIDON_FREQ_PARTIAL=$v -I$R/include \
        -Rpass-analysis=kernel-resource-usage -c $C/$f.hip -o $R/build_ab/${f}_pfq$v.o 2>> $R/build_ab/pfq${v}_resources.txt
    done
    objs=""
    for o in $C/*.o; do b=$(basename $o .o); if [ -f $R/build_ab/${b}_pfq$v.o ]; then objs="$objs $R/build_ab/${b}_pfq$v.o"; else objs="$objs $o"; fi; done
    $HIPCC -shared -fPIC --offload-arch=gfx950 -o $R/0-kno-vectorx_amd/libvx_pfq$v.so $objs
  done
  exit 0
fi
O=${VX_AB_OUT:-$R/build_ab/out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
for v in 0 1; do timeout -k 10 120 $R/build_ab/poseidon_rate_fq$v; done | tee $O/ab_poseidon_freq_micro.txt
[ "$(grep -o '"checksum": "[0-9a-f]*"' $O/ab_poseidon_freq_micro.txt | sort -u | wc -l)" = 1 ] || { echo "checksums differ"; exit 1; }
BASE=${VX_AB_BASE:-$R/0-kno-vectorx_amd/libvx_pfq0.so}
for round in 1 2 3; do
  for v in base 1; do
    if [ $v = base ]; then export VX_LIB_PATH=$BASE; else export VX_LIB_PATH=$R/0-kno-vectorx_amd/libvx_pfq1.so; fi
    timeout -k 10 300 python3 $R/bench.py --gpus 1 --steps 20 --warmup 5 > $O/ab_pfq_${v}_$round.json 2>/dev/null
    python3 -c "import json; d=json.loads([l for l in open('$O/ab_pfq_${v}_$round.json') if l.startswith('{')][-1]); print('round $round freq=$v: proofs/s', d['value'], 'ms per proof', d['ms_per_step'])"
  done
done | tee $O/ab_poseidon_freq_bench.txt
