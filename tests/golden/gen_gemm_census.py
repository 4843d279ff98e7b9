"""Record the GEMM launch census: tests/golden/gemm_launch_census.json.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_gemm_census.py [OUT.json]
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_gemm_census.py --add-missing
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_gemm_census.py --dispatches

Needs an MI355X and the built libraries.  It runs every case of tests/test_gpu_gemm_census.py (the
table and the runner live there) once and writes, per case and kernel name, the launch count and the
flops and bytes the launchers booked.  The committed table was recorded on the commit before the
launchers were rewritten over csrc/sr_gemm_plan.h, so that test pins the bookings that existed; record
it again only when a change is MEANT to alter them.  --add-missing runs only the cases the committed
table does not hold yet and adds their rows, leaving every recorded row as it is (the rows of the
timing-only variants were added that way, with the parent commit's libraries selected through
SUPER_RAG_AMD_LIB / SUPER_RAG_AMD_DIAG_LIB).

--dispatches writes no table: it runs the same cases plus the pair around the automatic persistent
threshold (N 256, K 128, M 130,816 and 130,817), as the driver of a kernel trace whose (kernel, grid,
workgroup, LDS) lists two builds are compared by (SUPER_RAG_AMD_LIB / SUPER_RAG_AMD_DIAG_LIB select
the build).
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
    import test_gpu_gemm_census as C
    args = sys.argv[1:]
    dispatches = "--dispatches" in args
    add_missing = "--add-missing" in args
    args = [a for a in args if a not in ("--dispatches", "--add-missing")]
    out = args[0] if args else C.GOLDEN
    table = {}
    if add_missing:
        with open(C.GOLDEN) as f:
            table = json.load(f)
    if dispatches:
        for m in (130816, 130817):
            C.CASES["gemm_auto_threshold_%d" % m] = ("gemm", (-1, 0, m, 256, 128))
    for name in C.CASES:
        if name in table:
            continue
        table[name] = C.run_case(name, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
    print(len(table), "cases,", sum(v["launches"] for t in table.values() for v in t.values()),
          "booked launches", flush=True)
    if dispatches:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        rows = ['"%s": %s' % (k, json.dumps(table[k], sort_keys=True)) for k in sorted(table)]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")   # one case per line


if __name__ == "__main__":
    main()
