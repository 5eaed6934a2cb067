cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
D=${1:?usage: tools/gpu_run1.sh <output directory>}
mkdir -p "$D"
t0=$(date +%s)
python bench.py --full > "$D/bench_default.json" 2> "$D/bench_default.err"
t1=$(date +%s)
echo "bench.py --full wall: $((t1-t0)) s"
tail -3 "$D/bench_default.err"
D="$D" python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['D'], 'bench_default.json')).read().strip().split('\n')[-1])
print({k:(v if not isinstance(v,dict) else {kk:vv for kk,vv in v.items() if kk in ('value','frac','achieved','ms_per_step','kind','cores','unit','max_mem_gb','dtype')}) for k,v in d.items() if k not in ('config','metric','data')})
PY
