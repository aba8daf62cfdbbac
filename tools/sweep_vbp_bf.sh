# vbp best-fit config-5 sweep: window sizes x band list segments (PVT_BAND_SEGS), parity checked
for w in 512 1024; do for sg in 16; do
log=$(mktemp -t sw_${w}_${sg}.XXXXXX)
PVT_BAND_SEGS=$sg timeout -k 10 120 python bench.py --mode vbp_bf --window $w --full --extra 0 --replay 0 --cpu-baseline-seconds 0 > "$log" 2>&1 || { echo "failed: $log"; exit 1; }
tail -1 "$log" | python -c "
import json,sys; d=json.loads(sys.stdin.read()); print('w=$w S=$sg', round(d['ms_per_step'],3), d['parity'], {k: round(v,3) for k,v in d['kernels_ms_per_step'].items()}, d.get('windows_per_step'), d.get('refills_per_step'))"
done; done
