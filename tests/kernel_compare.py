"""A comparison of a kernel's output with its f64-accumulated reference that localises: where tests/test_kernels_gpu.py::close() is one global
relative L2, compare() also bounds every row, every column and every single element, and checks that nothing outside the output was written.
A helper, not a test module; its own tests are tests/test_kernel_compare.py (CPU).

Why a per-element bound can be asserted without a measured number: kernel and reference start from the same operand values and both round
their result once to the storage type, so they land on the same grid.  The exact result v, the reference's ref = round(v (1 + ~2^-53)) and the
kernel's got = round(v + e) differ by at most one unit of that grid plus the kernel's f32 accumulation error e.  A sequential f32 evaluation of
K products (exact in f32 for 16-bit operands) and the handful of epilogue terms makes at most K + 8 roundings of relative size 2^-24, each
acting on a partial sum of magnitude at most S = sum of the absolute values of all terms (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1: |e| <= gamma_n sum |x_i y_i|), hence
    |got - ref| <= ulp_T(ref) + C_ACC (K + 8) 2^-24 S
with C_ACC = 1.  Any other summation order (the matrix instructions add 4 / 16 / 32 products at a time, the K slices of split-K are added
afterwards) has FEWER roundings on the path of a term than the sequential one, so it stays under the same bound.
"""
from collections import namedtuple

import torch

RTOL = {"bf16": 4e-3, "f32": 2e-5, "f16": 5e-4}      # the project's tolerances (tests/test_kernels_gpu.py::RTOL)
FRAC_BITS = {"bf16": 7, "f16": 10, "f32": 23}
MIN_EXP = {"bf16": -126, "f16": -14, "f32": -126}     # exponent of the smallest normal number: below it the spacing stays that of the subnormals

# c of the bound above.  1 is the derived value for a sequential f32 sum; no case measured on the MI355X needed more (the worst
# per-element error / bound ratios are in profiles/gemm_epilogue_coverage.txt), so it was never raised.
C_ACC = 1.0

# S: [rows][columns] f64, the sum of the absolute values of every term the epilogue adds, times |out_scale| (gemm_cases.bound_terms);
# K: length of the dot product; tile: (rows, columns) of the executed tile, for the report only
BoundTerms = namedtuple("BoundTerms", ["S", "K", "tile"], defaults=[(128, 128)])
# before / after: the whole output buffer (guard bands included) before and after the launch; mask: True where the op may write
Guard = namedtuple("Guard", ["before", "after", "mask"])

last_figures = {}      # the figures of the latest compare() call, for the tests that record them


def ulp(x, dtype):
    """spacing of the storage type at |x| (x: f64 tensor)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** MIN_EXP[dtype])))
    return torch.exp2(e.clamp_min(MIN_EXP[dtype]) - FRAC_BITS[dtype])


def element_bound(ref, dtype, bound_terms):
    return ulp(ref, dtype) + C_ACC * (bound_terms.K + 8) * 2.0 ** -24 * bound_terms.S.double()


def _where(i, j, tile, prefix=""):
    bm, bn = tile
    return (f"{prefix}row {i}, column {j} (row tile {i // bm} of {bm} rows, row {i % bm} in it; column tile {j // bn} of {bn} columns, column {j % bn} in it; "
            f"16-row pass {i % bm // 16}, lane column {j % 16})")


def _bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def compare(got, ref, *, dtype, bound_terms, guard=None, tag):
    """got, ref: [rows][columns], the kernel's output window and the reference from EmuOps(acc=torch.float64), both in the storage type `dtype`
    ("bf16" / "f16" / "f32").  Asserts, in this order: (a) finite everywhere, (b) global relative L2 <= RTOL[dtype], (c) relative L2 of every row and
    of every column <= RTOL[dtype] (rows / columns whose reference norm is below the norm of their per-element bounds are left to (d)),
    (d) every element within element_bound(), (e) everything outside guard.mask bit-identical.  No element is exempt from (d)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    assert g.dim() == 2 and g.shape == r.shape == tuple(bound_terms.S.shape), (tag, g.shape, r.shape, tuple(bound_terms.S.shape))
    tile, rtol = bound_terms.tile, RTOL[dtype]
    fig = last_figures
    fig.clear()
    fig.update(tag=tag, dtype=dtype)
    # (a)
    nonfin = (~torch.isfinite(g)).nonzero()
    assert nonfin.numel() == 0, f"{tag}: {nonfin.shape[0]} non-finite values, first at {_where(*nonfin[0].tolist(), tile)}"
    diff = g - r
    bound = element_bound(r, dtype, bound_terms)
    ratio = diff.abs() / bound
    worst = int(ratio.argmax())
    wi, wj = divmod(worst, g.shape[1])
    # (b)
    rel = (diff.norm() / (r.norm() + 1e-300)).item()
    fig.update(global_rel=rel, elem_ratio=ratio.max().item())
    assert rel <= rtol, f"{tag}: global rel-L2 {rel:.3e} > {rtol:.1e}; worst element {ratio.max().item():.3g} x its bound at {_where(wi, wj, tile)}"
    # (c)
    for axis, what in ((1, "row"), (0, "column")):
        rn, dn, bnorm = r.norm(dim=axis), diff.norm(dim=axis), bound.norm(dim=axis)
        judged = rn > bnorm
        rel_ax = torch.where(judged, dn / rn.clamp_min(1e-300), torch.zeros_like(dn))
        fig[what + "_rel"] = rel_ax.max().item()
        bad = (rel_ax > rtol).nonzero().reshape(-1)
        if bad.numel():
            k = int(bad[0])
            line = diff[k] if axis == 1 else diff[:, k]
            o = int(line.abs().argmax())
            i, j = (k, o) if axis == 1 else (o, k)
            raise AssertionError(f"{tag}: {what} {k} rel-L2 {rel_ax[k].item():.3e} > {rtol:.1e} ({bad.numel()} {what}s over); its worst element: got {g[i, j].item():.6g}, "
                                 f"ref {r[i, j].item():.6g} at {_where(i, j, tile)}")
    # (d)
    over = (diff.abs() > bound).nonzero()
    if over.numel():
        i, j = over[0].tolist()
        raise AssertionError(f"{tag}: {over.shape[0]} of {g.numel()} elements outside |got - ref| <= ulp + {C_ACC:g} (K + 8) 2^-24 S; first: got {g[i, j].item():.8g}, "
                             f"ref {r[i, j].item():.8g}, |diff| {abs(diff[i, j].item()):.3e} = {ratio[i, j].item():.3g} x bound {bound[i, j].item():.3e} at {_where(i, j, tile)}; "
                             f"worst {ratio.max().item():.3g} x at {_where(wi, wj, tile)}")
    # (e)
    if guard is not None:
        before, after, mask = _bits(guard.before), _bits(guard.after), guard.mask.detach().cpu().reshape(-1)
        assert before.shape == after.shape == mask.shape, (tag, before.shape, after.shape, mask.shape)
        touched = ((before != after) & ~mask).nonzero().reshape(-1)
        if touched.numel():
            first_out = int(mask.nonzero()[0])
            k = int(touched[0])
            raise AssertionError(f"{tag}: {touched.numel()} elements outside the output were written; first at buffer element {k} "
                                 f"({k - first_out:+d} from the first output element; was {guard.before.reshape(-1)[k].item()!r}, is {guard.after.reshape(-1)[k].item()!r})")
    return dict(fig)
