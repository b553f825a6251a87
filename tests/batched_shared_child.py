"""Child process of tests/test_gpu_batched_shared.py: one case of its table, shared against stacked, in a process of its
own (the workgroup width is chosen from MADQP_BATCH_WIDE_MAX, which the library reads once).  Exits non-zero on a mismatch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(name):
    import madqp_jl_amd as M
    import test_gpu_batched_shared as T

    be = M.HipBackend(0)
    try:
        _, stacked, shared = T.both(be, name)
        for b, (r0, r1) in enumerate(zip(stacked, shared)):
            T.assert_same_bits(r0, r1, (name, b))
        assert all(r["status"] == M.SOLVE_SUCCEEDED for r in shared), [r["status"] for r in shared]
    finally:
        be.close()
    print(f"narrow programs: shared == stacked on {name} ({len(shared)} problems, MADQP_BATCH_WIDE_MAX="
          f"{os.environ.get('MADQP_BATCH_WIDE_MAX')})")


if __name__ == "__main__":
    main(sys.argv[1])
