"""The launch trace of `mtvaf_amd.optim.AdamW` (tests/optim_trace.py) against tests/golden/adamw_launch_trace.json.

    python tools/adamw_trace.py            # run the scenarios on the GPU, compare with the file, exit 1 on a difference
    python tools/adamw_trace.py --write    # regenerate the file (on the commit whose launches are the reference)
    python tools/adamw_trace.py --out F    # write the trace to F instead (two runs of one tree must give identical files)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import optim_trace as T
    text = T.dumps(T.run_scenarios())
    if a.write or a.out:
        path = a.out or T.GOLDEN
        with open(path, "w") as f:
            f.write(text)
        print(f"{path}: {text.count(chr(10)) - 1} lines, {len(text)} bytes")
        return 0
    with open(T.GOLDEN) as f:
        same = f.read() == text
    print("the trace is the recorded one" if same else "the trace DIFFERS from the recorded one (--out F, then diff)")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
