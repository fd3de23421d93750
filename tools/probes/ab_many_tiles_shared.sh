# one panorama of 24 / 64 4K tiles in a row on one GPU: one deferred chain over a device tile table (default) against the column strips (ISX_TAB=0),
# with the per-kernel times and the host's enqueue time
P='import sys,json
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d["roofline"]; k=d["kernels_ms_one_step"]
print(d["value"], d["ms_per_step"], "host_enqueue_ms_per_pair", d["config"]["host_enqueue_ms_per_pair"], d["config"].get("path"), {n: v["ms"] for n, v in k.items()})'
# (host_enqueue_ms_per_pair comes with --full); results under the directory given as $1, default the current one
O=${1:-.}; mkdir -p $O
for rep in 1 2; do
for args in "--tiles 24 --focal 9000 --yaw 0.12" "--tiles 64 --focal 24000 --yaw 0.046"; do
for v in ISX_TAB=1 ISX_TAB=0; do
  echo -n "[$v] $args : " >> $O/ab_many_tiles_shared.txt
  env $v timeout 600 python bench.py $args --full --steps 6 --warmup 2 --no-dropin --no-cpu-baseline --no-live-traffic 2> $O/ab_many_tiles.err | python -c "$P" >> $O/ab_many_tiles_shared.txt 2>&1
done; done; done
cat $O/ab_many_tiles_shared.txt
