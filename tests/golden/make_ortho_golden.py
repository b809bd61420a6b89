"""Writes tests/golden/ortho_fused_hashes.json: per case of tests/test_ortho_fused_gpu.py the SHA-256 of Qo, Yb and T as
dlco_ortho_probe returns them with unfused = 1, i.e. from the separate launches (symmetric product + ordered reduce, Gram
GEMM + ordered reduce, Cholesky inverse, L^-1 GEMM).  Needs an MI355X.

The committed file was taken from the commit BEFORE the fused reductions existed: its kernels, its gemm_f32 /
splitk_reduce_f32 / skinny_product_sym and its EigTracker::product / gram_rect / orthonormalize, with nothing added but
the probe entry itself (dlco_ortho_probe calling those members in the tracker's order; that commit has no other form, so
`unfused` is ignored there).  To repeat that, check out that commit, add the probe entry and this script with the test
module, build, and run
    python tests/golden/make_ortho_golden.py [OUT.json]
Run on a later commit it records that commit's unfused launches instead, which the test holds equal to the committed
hashes anyway."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch  # noqa: F401  (first HIP runtime in the process, as in tests/conftest.py)
    dlco = importlib.import_module("opencv-dlco_amd")
    import test_ortho_fused_gpu as t

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ortho_fused_hashes.json")
    ctxs, golden = {}, {}
    for name in sorted(t.CASES):
        F = t.CASES[name][0]
        if F not in ctxs:
            ctxs[F] = dlco.Context(F, 16, B=4)
        Z, Zprev, Gp = t.inputs(name)
        r = ctxs[F].ortho_probe(Z, Gp, t.ALPHA, t.B1, t.B2, Zprev=Zprev, unfused=True)
        assert r["fused"] == 0
        golden[name] = t.digest(r)
        print(name, golden[name]["T"][:16])
    for c in ctxs.values():
        c.close()
    with open(out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
