"""Outputs of the general circular-OT path (n != m and / or weights) over a fixed case list, for bit-for-bit comparison
of two builds of the library.

    SHW_LIB_PATH=/path/to/libshw_hip.so python tools/general_outputs.py OUT.pt     run the cases with that library
    python tools/general_outputs.py --compare A.pt B.pt                            every tensor bit for bit; exit 1 on a mismatch

One process per library (the library is loaded once per process).  The cases: one shape per size class of the general
kernels, at the class's top, B = 2 pairs and L = 8 slices; with and without per-pair weights; p = 2 and 3 through
shw_ssw_forward_general, p = 1 through shw_circle_ot's bisection (the cut search at p = 1) and, with weights, through
shw_ssw_forward_general (the level median); loss only and loss with gradient coefficients.  Kept per case: the slice
costs, the cuts the solve ended on, and both coefficient rows (d cost / d circle coordinate of either cloud).  These
kernels are deterministic (owner-computed coefficients, sums in a fixed order), so two builds that compute the same
thing agree in every bit.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 50), (128, 100), (256, 200), (512, 400), (1024, 768), (2048, 1536), (4096, 3000)]
B, L = 2, 8


def run(out_path):
    from shw_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    out = {}
    for n, m in SHAPES:
        g = torch.Generator().manual_seed(1100 + n)
        x = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1).to(dev)
        y = torch.nn.functional.normalize(torch.randn(B, m, 3, generator=g), dim=-1).to(dev)
        U = torch.linalg.qr(torch.randn(B, L, 3, 2, generator=g))[0].contiguous().to(dev)
        u, v = torch.rand(B * L, n, generator=g).to(dev), torch.rand(B * L, m, generator=g).to(dev)

        def weights(rows, count):
            w = torch.rand(rows, count, generator=g) + 0.05
            return (w / w.sum(1, keepdim=True)).to(dev)
        for weighted in (False, True):
            wu, wv = (weights(B, n), weights(B, m)) if weighted else (None, None)           # per pair
            ru, rv = (weights(B * L, n), weights(B * L, m)) if weighted else (None, None)   # per row
            for grad in (False, True):
                for case in ("p2", "p3", "p1", "circle p1"):
                    if case == "p1" and not weighted:
                        continue                    # (no weights at p = 1 is not the general path)
                    # poisoned outputs: a word the kernels leave unwritten shows as a difference between two runs' NaN patterns
                    cost = torch.full((B * L,), float("nan"), device=dev)
                    cut = torch.full((B * L,), float("nan"), device=dev)
                    cs = torch.full((B * L, n), float("nan"), device=dev) if grad else None
                    ct = torch.full((B * L, m), float("nan"), device=dev) if grad else None
                    if case == "circle p1":
                        _lib.check(lib.shw_circle_ot(ptr(u), ptr(v), ptr(ru), ptr(rv), n if weighted else 0, m if weighted else 0,
                                                     B * L, n, m, 1.0, _lib.CIRCLE_BISECTION, ptr(cost), ptr(cut), ptr(cs),
                                                     ptr(ct), stream), "shw_circle_ot")
                    else:
                        _lib.check(lib.shw_ssw_forward_general(ptr(x), ptr(y), ptr(U), ptr(wu), ptr(wv), n if weighted else 0,
                                                               m if weighted else 0, B, n, m, L, L * 6, float(case[1:]),
                                                               ptr(cost), ptr(cut), ptr(cs), ptr(ct), stream),
                                   "shw_ssw_forward_general")
                    key = "n%d m%d w%d %s grad%d" % (n, m, weighted, case, grad)
                    out[key + " cost"], out[key + " cut"] = cost.cpu(), cut.cpu()
                    if grad:
                        out[key + " coef_s"], out[key + " coef_t"] = cs.cpu(), ct.cpu()
    torch.save(out, out_path)
    finite = sum(bool(torch.isfinite(t).all()) for t in out.values())
    print("%s: %d tensors (%d all finite) of %d cases with %s" % (out_path, len(out), finite,
                                                                  len({k.rsplit(" ", 1)[0] for k in out}), _lib.LIB_PATH))


def compare(path_a, path_b):
    a, b = torch.load(path_a), torch.load(path_b)
    # (bit patterns, so that a NaN equals itself)
    bad = sorted(set(a) ^ set(b)) + [k for k in sorted(set(a) & set(b)) if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    for k in bad:
        print("MISMATCH", k)
    print("tensors compared: %d, not bit-identical: %d" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2:
        run(sys.argv[1])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
