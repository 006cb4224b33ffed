#!/bin/bash
# One first stage per pass (R0 = 18, 20) against the run-time pass, same box, harness builds made beforehand with
#   build.sh -o p20 -DWF_ONLY_R0=20 -DWF_PASS_SPLIT=0                          (the code before the split)
#   build.sh -o s20 -DWF_ONLY_R0=20 -DWF_SEED_DERIVE=0 -DWF_TWIST_FOLD=0       (split only)
#   build.sh -o st20 -DWF_ONLY_R0=20 -DWF_SEED_DERIVE=0                        (+ twist inside the butterfly)
#   build.sh -o a20 -DWF_ONLY_R0=20                                            (+ squared seeds: the library's code)
#   build.sh -o f20 -DWF_ONLY_R0=20 -DWF_SEED_DERIVE=3                         (one seed request in both passes)
# and p18 / a18 the same for R0 = 18.  Check of both passes, 250 launches of 24 GB per run (one warm-up run discarded),
# ROUNDS rounds over the variants, then stamped runs (cycles per unit and pass for S1 / S2, in-kernel clock).
# Every step under its own time limit; the first failure ends the script.  -> profiles/r08_headline_ab.txt
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${1:-$R/profiles/r08_pass_split_raw.txt}
ROUNDS=${ROUNDS:-5}
mkdir -p "$(dirname "$OUT")"
run() { echo "### $*"; "$@" || { echo "### failed: stopping"; exit 1; }; }
{
echo "# pass_split_report.sh $(date -u +%FT%TZ)"
run env WF_R0=20 timeout -k 10 120 $R/tools/wfft/wfft_test_a20 check
run env WF_R0=18 timeout -k 10 120 $R/tools/wfft/wfft_test_a18 check
run env WF_R0=20 timeout -k 10 120 $R/tools/wfft/wfft_test_p20 time 150000 10000 250 0
for round in $(seq $ROUNDS); do
  for v in p20 s20 st20 a20 f20; do
    echo "## round $round wfft_test_$v (sha $(sha256sum $R/tools/wfft/wfft_test_$v | cut -c1-16))"
    run env WF_R0=20 timeout -k 10 120 $R/tools/wfft/wfft_test_$v time 150000 10000 250 0
  done
  for v in p18 a18; do
    echo "## round $round wfft_test_$v (sha $(sha256sum $R/tools/wfft/wfft_test_$v | cut -c1-16))"
    run env WF_R0=18 timeout -k 10 120 $R/tools/wfft/wfft_test_$v time 150000 9216 250 0
  done
done
for v in p20 a20 p20 a20; do
  echo "## stamped wfft_test_$v"
  run env WF_R0=20 timeout -k 10 120 $R/tools/wfft/wfft_test_$v time 150000 10000 250 1
done
} 2>&1 | tee "$OUT"
exit ${PIPESTATUS[0]}
