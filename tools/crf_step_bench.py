"""bench.py's training step with a tag set of another size: the model is built with a label list of TAGS - 1 entries
(TVNetSAModel2 adds one tag), so the CRF runs with C = TAGS; everything else is bench.py as it stands (labels stay in
[1, 11), valid for any C >= 11).
    python tools/crf_step_bench.py TAGS [bench.py arguments ...]
e.g.  python tools/crf_step_bench.py 21 --gpus 1 --steps 40 --warmup 5"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
os.chdir(ROOT)

import bench  # noqa: E402

tags = int(sys.argv[1])
if tags < 11:
    raise SystemExit("TAGS must be at least 11 (bench.py draws labels from [1, 11))")
bench.LABELS = bench.LABELS + [f"EXTRA-{i}" for i in range(tags - 1 - len(bench.LABELS))]
sys.argv = ["bench.py"] + sys.argv[2:]
bench.main()
