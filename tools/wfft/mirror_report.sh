#!/bin/bash
# Mirrored first-stage output twiddles (R0 = 18, 20) against both chains run to R0 - 1, same box, harness builds made
# beforehand with
#   build.sh -o m0_20 -DWF_ONLY_R0=20 -DWF_TWIDDLE_MIRROR=0     (the code before)
#   build.sh -o m1_20 -DWF_ONLY_R0=20                           (chains to R0/2: the library's code)
#   build.sh -o f_20 -DWF_ONLY_R0=20 -DWF_SEED_DERIVE=3         (+ pass 1 squares g for g2: one seed request in both passes)
# and m0_18 / m1_18 / f_18 the same for R0 = 18.  Check of both passes, 250 launches of 24 GB per run (one warm-up run
# discarded), five rounds over the variants (R0 = 18: three), then stamped runs (cycles per unit and pass for S1 / S2,
# in-kernel clock).  Every step under its own time limit; the first failure ends the script.  -> profiles/r09_headline_ab.txt
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${1:-$R/profiles/r09_mirror_raw.txt}
ROUNDS=${ROUNDS:-5}
W=$R/tools/wfft
mkdir -p "$(dirname "$OUT")"
run() { echo "### $*"; "$@" || { echo "### failed: stopping"; exit 1; }; }
{
echo "# mirror_report.sh $(date -u +%FT%TZ)"
run env WF_R0=20 timeout -k 10 120 $W/wfft_test_m1_20 check
run env WF_R0=18 timeout -k 10 120 $W/wfft_test_m1_18 check
run env WF_R0=20 timeout -k 10 120 $W/wfft_test_m0_20 time 150000 10000 250 0
for round in $(seq $ROUNDS); do
  for v in m0_20 m1_20 f_20; do
    echo "## round $round wfft_test_$v (sha $(sha256sum $W/wfft_test_$v | cut -c1-16))"
    run env WF_R0=20 timeout -k 10 120 $W/wfft_test_$v time 150000 10000 250 0
  done
  [ $round -le 3 ] || continue
  for v in m0_18 m1_18 f_18; do
    echo "## round $round wfft_test_$v (sha $(sha256sum $W/wfft_test_$v | cut -c1-16))"
    run env WF_R0=18 timeout -k 10 120 $W/wfft_test_$v time 150000 9216 250 0
  done
done
for v in m0_20 m1_20 f_20 m0_20 m1_20 f_20; do
  echo "## stamped wfft_test_$v"
  run env WF_R0=20 timeout -k 10 120 $W/wfft_test_$v time 150000 10000 250 1
done
} 2>&1 | tee "$OUT"
exit ${PIPESTATUS[0]}
