set -u
# usage: bash tools/gpu_check6.sh [output directory]
O=${1:-build/c1}; mkdir -p "$O"
timeout -k 10 700 python -u -m pytest -x -q --timeout 200 --timeout-method thread -p no:cacheprovider tests/test_gpu_round6.py tests/test_gpu_round2.py tests/test_gpu_wls.py tests/test_gpu_parity.py tests/test_gpu_round5.py tests/test_gpu_wta.py > "$O/t.log" 2>&1; rc=$?
tail -2 "$O/t.log"; [ $rc -gt 1 ] && exit $rc
timeout -k 10 300 python3 tools/single_pair.py --calls 30 --stages call --runs "0;0" > "$O/sp1.log" 2>&1 || exit 3
timeout -k 10 300 python3 tools/single_pair.py --calls 30 --stages call,h2d,d2h --runs "0;0" > "$O/sp2.log" 2>&1 || exit 3
grep -h "^{" "$O/sp1.log" "$O/sp2.log" | cut -c1-60,200-400
timeout -k 10 300 python -u bench.py --full --steps 200 --warmup 10 --cpu-baseline-pairs 0 > "$O/b.log" 2>&1 || exit 3
python3 -c "
import json, sys; l=[x for x in open(sys.argv[1]) if x.startswith('{')][-1]; d=json.loads(l); hs=d['host_surface']; s=d['stage_us_per_pair']
print(d['value'], {k: round(v,1) for k,v in s.items() if v}); print(hs['value'], hs['ms_per_call_median'], hs['device_ms_per_call'], hs['one_call_abi']['device_ms_per_call'], hs['one_call_abi']['value'])" "$O/b.log"
