"""Bitwise comparison of two builds of libqoc_mi355x.so on the small cases of tests/test_gpu_blkseg_peel.py (every
boundary of the segmented eval's slice loops, the series classes, halvings, orders 1 / 3 / exact, the penalty, blocks of
3 rows, fused and split) and of tests/blkseg_util.py's shipped cases (zz, cavity20, cavity40: order 3 and exact, with
and without their penalties).  Needs an MI355X.
  QOC_LIB_PATH=/path/to/other/libqoc_mi355x.so python tools/blkseg_bits.py dump a.npz
  python tools/blkseg_bits.py dump b.npz
  python tools/blkseg_bits.py cmp a.npz b.npz        (exit status 1 when an array differs)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "quantumoptimalcontrol.jl_amd", ""):
    sys.path.insert(0, os.path.join(ROOT, p))


class Env:
    """The part of pytest's monkeypatch that tests/blkseg_util.engine uses."""
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def dump(path):
    import torch
    torch.cuda.init()  # torch's HIP runtime first, then the library's (tests/conftest.py built_lib)
    torch.empty(1, device="cuda")
    import blkseg_util as U
    import test_gpu_blkseg_peel as T
    out = {}

    def run(tag, prob, u, orders, S=None, penalty=None):
        e = U.engine(prob, u.shape[0], Env(), pen=penalty, S=S)
        for order in orders:
            for form, fn in (("fused", U.eval_dev), ("split", U.split_dev)):
                J, g = fn(e, np.asarray(u), order)
                out[f"{tag}/{order}/{form}/J"], out[f"{tag}/{order}/{form}/dJdu"] = J, g
        e.close()

    pen20 = U.pen(U.case("cavity20")[2])
    for Nt, S, _, _ in T.SHAPES:
        for cls in T.AMPS:
            run(f"cavity/Nt{Nt}/S{S}/{cls}", *T.cavity(Nt, cls), [3], S=S)
        run(f"cavity/Nt{Nt}/S{S}/orders", *T.cavity(Nt), [1, "exact"], S=S)
    for Nt, S in T.LF_KINDS:
        run(f"cavity/Nt{Nt}/S{S}/pen", *T.cavity(Nt), [3, "exact"], S=S, penalty=pen20)
        run(f"blocks3/Nt{Nt}/S{S}", *T.blocks3(Nt)[:2], [3, "exact"], S=S)
    for name in ("zz", "cavity20", "cavity40"):
        prob, u, pn = U.case(name)
        run(name, prob, u, [3, "exact"])
        run(name + "/pen", prob, u, [3, "exact"], penalty=U.pen(pn))
    np.savez(path, **out)
    print(len(out), "arrays ->", path)


def cmp(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = [k for k in A.files if k not in Bz.files or not np.array_equal(A[k], Bz[k])]
    bad += [k for k in Bz.files if k not in A.files]
    for k in bad:
        print("DIFFERS", k)
    print(len(A.files), "arrays,", len(bad), "differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
