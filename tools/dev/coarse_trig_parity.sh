#!/bin/bash
# developer check (GPU box): bench.py's c2f parity block (4096-ray renders against the oracle on 256 of the rays; seed and in-run trained parameters) with the
# coarse level's hardware sines (default) and with the polynomial (EVD_COARSE_TRIG=exact)
O=${1:?usage: tools/dev/coarse_trig_parity.sh OUTPUT_DIR}; mkdir -p "$O"
for t in rev exact; do
  EVD_COARSE_TRIG=$t python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-train --no-modes --no-composite --no-awp --no-strong --no-zero-probe > "$O/trig_$t.json" 2> "$O/trig_$t.err"
done
python - "$O" <<PY > "$O/coarse_trig_parity.log"
import json, os, sys
for t in ("rev", "exact"):
    d = json.loads(open(os.path.join(sys.argv[1], "trig_%s.json" % t)).read().strip().splitlines()[-1])["c2f"]
    p = d["parity"]["rgb_linf_vs_oracle"]
    print(t, "c2f ms", round(d["ms_per_step"], 4), {k: v.get("f16c") for k, v in p.items()})
PY
