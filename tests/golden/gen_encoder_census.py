"""Record the encoder launch census: tests/golden/encoder_launch_census.json.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_encoder_census.py [OUT.json]

Needs an MI355X and the built library.  It runs every configuration of
tests/test_gpu_encoder_census.py (the table and the runner live there) once and writes, per
configuration and kernel name, the launch count and the flops and bytes the launchers booked.  The
committed table was recorded on the commit before Encoder::forward_dev was split into stages, so
that test pins the launch sequence that existed; record it again only when a change is MEANT to
alter the launches, on the commit before that change's host-side follow-ups.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "super-rag_amd"), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("SUPER_RAG_AMD_SYNTHETIC", "1")


def main():
    import test_gpu_encoder_census as C
    out = sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN
    table = {}
    for name in C.CONFIGS:
        table[name] = C.run_census(name, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        print(name, sum(v["launches"] for v in table[name].values()), "launches", flush=True)
    for k in C.SWITCHES:
        os.environ.pop(k, None)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
