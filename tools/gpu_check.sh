#!/bin/bash
# tools/gpu_check.sh <tag> <output dir>: the -m gpu suite, smoke() and the full bench line (bench.py --full) into <output dir>/<tag>_*
export TMPDIR=/tmp
TAG=${1:-r03}
OUT=${2:?usage: tools/gpu_check.sh <tag> <output dir>}
mkdir -p "$OUT"
timeout 2400 python -m pytest tests -m gpu -q -s > "$OUT/${TAG}_pytest.log" 2>&1; echo "pytest rc=$?"; tail -3 "$OUT/${TAG}_pytest.log"
grep -h "pivots differing" "$OUT/${TAG}_pytest.log"
timeout 300 python -c "import __graft_entry__ as g; g.build(); g.smoke()" 2>&1 | tail -2
timeout 900 python bench.py --steps 20 --warmup 3 --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"; echo "bench rc=$?"
python - <<PY
import json
d=json.loads([l for l in open('$OUT/${TAG}_bench.json') if l.startswith('{')][-1])
print({k:d.get(k) for k in ('value','n_gpus','steps','ms_per_step','scaling','value_incl_h2d','value_resident')})
print(d['roofline']['frac'], d['tsqr'].get('seconds'), d['tsqr'].get('executed_frac_of_fp64_mfma_peak'), d['cpu_baseline']['value'], d.get('parity'))
print(json.dumps(d.get('kernel_ms_per_step')))
PY
