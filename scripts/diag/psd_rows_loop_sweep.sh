# The rows loop of the 64k PSD (psdfft.hip psd_rows_pk_kernel) on the C3 step: grid rows R (half and the whole of the residency
# of a 256-CU device, and the plan's evened default) x streams, beside the unit form; the columns pass stays the default loop.
#   scripts/diag/psd_rows_loop_sweep.sh [repeats]
for rep in $(seq ${1:-2}); do
for streams in 1 2; do
for path in rows=unit rows=loop:32 rows=loop:64 default; do
  if [ $path = default ]; then unset PYSDR_PSD_PATH; else export PYSDR_PSD_PATH=$path; fi
  PYSDR_TUNING=1 PYSDR_PSD_STREAMS=$streams timeout -k 10 120 python bench.py --steps 30 --warmup 5 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
print('pass $rep streams $streams path %-12s' % '$path', 'GS/s %.1f' % (d['value'] / 1e3), 'ms %.4f' % d['ms_per_step'])" || exit 1
done
done
done
