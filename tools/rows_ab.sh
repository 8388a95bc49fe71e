#!/bin/bash
# development A/B of saf_window.hip compile-time options on one box: bash tools/rows_ab.sh "<-D flags>[;ENV=..]" ...
run() { for k in A B; do env $2 timeout -k 10 200 python3 bench.py --full --cpu-frames 0 --no-side --end-to-end 0 --steps 3 --warmup 1 --depth-kind $k 2>/dev/null | python3 -c "
import sys,json
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d['roofline']
print('$1 $2', 'depth $k:', d['value'], 'frames/s', d['ms_per_step'], 'ms; rows', r['avg_launch_us'], 'alone', (r.get('isolated') or {}).get('avg_launch_us'), 'classify', d['kernel_breakdown']['sweep_us'])"; done; }
run "default" "SAF_X=1"
for spec in "$@"; do
  f="${spec%%;*}"; e="${spec#*;}"; [ "$e" = "$spec" ] && e="SAF_X=1"
  (cd spatially_aware_ai_amd/csrc && touch saf_window.hip && make HIPFLAGS="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC $f" > /dev/null 2>&1) && run "$f" "$e"
done
