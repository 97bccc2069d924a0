D=${1:?usage: bash tools/tune_in_flight_ab.sh <output dir>}; mkdir -p $D
for rep in 1 2; do
for mode in "--no-tune-in-flight" ""; do
  rm -f $D/tc.txt
  DC_TUNE_CACHE=$D/tc.txt python bench.py --full --no-cpu-baseline --no-f16-line --no-resnet101 --coalesce 0 --steps 60 --warmup 5 $mode 2>>$D/err.txt | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('f32 [%s]' % '$mode', round(d['value'],1), round(d['one_forward_at_a_time']['value'],1), d['config']['tile_tuning'])"
  rm -f $D/tc.txt
  DC_TUNE_CACHE=$D/tc.txt python bench.py --full --no-cpu-baseline --no-f16-line --no-resnet101 --coalesce 0 --dtype f16 --batch 8 --streams 2 --steps 30 --warmup 4 $mode 2>>$D/err.txt | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('f16 [%s]' % '$mode', round(d['value'],1), round(d['one_forward_at_a_time']['value'],1), d['config']['tile_tuning'])"
done; done
tail -5 $D/err.txt
