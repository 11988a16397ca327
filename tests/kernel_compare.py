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

Softmax attention (fyc_attention, fyc_temporal_attention) gets a bound of the same kind, derived from the kernels' rounding points; the reference is
plain f64 - scores s_j = scale q.k_j, weights w = softmax(s), o = sum_j w_j v_j - with NO rounding of the weights (softmax_bound_terms below; not
EmuOps.attention, which rounds P as the kernels do and so hides a kernel that rounds it wrongly).  u = 2^-9 (bf16), 2^-12 (f16), 2^-24 (f32).

Rounding points of the flash kernel (csrc/attention_kernel.h), T the 16-bit storage type:
  1. Q' = T(f32(q scale log2e)): one f32 product, one rounding to T per element;
  2. the score in log2 units: an f32 MFMA sum of d products of T values (exact in f32) - d roundings; under MSUB the slot of index d adds
     (-m) * 1 with m a T number: exact, no rounding of its own;
  3. s - m (not under MSUB), s - delta when the maximum moves: f32 subtractions; exp2 in f32 (v_exp_f32, 1 ulp);
  4. p = T(exp2(s - m)): one rounding to T.  p <= 2^6 between moves of the maximum, which changes nothing in relative terms;
  5. O^T += V^T P^T and l += 1 P^T: f32 MFMA sums over the n_k keys of products of T values, multiplied by alpha = exp2(m_old - m_new) (f32) on a move;
  6. o / l as o * (1 / l): two f32 roundings; one rounding to T at the store (o_accumulate: prev + o_scale * v in f32 - two roundings - then T).
Hence the score of key j is off by at most Es_j = (u + (d + 8) 2^-24) scale log2e sum_i |q_i| |k_ji| log2 units (u: point 1; d + 8: points 2, 3), the weight
the kernel gives key j is w_j (1 + e_j) with |e_j| <= eta_j = expm1(u + ln2 Es_j) (u: point 4) BEFORE normalisation, and as l is the sum of the very same
rounded p the normalised weights still add up to 1: their error moves the output only along v_j - o,
    |got - ref| <= ulp_T(ref) + sum_j w_j eta_j |v_j - o| / (1 - sum_j w_j eta_j) + (n_k + 8) 2^-24 sum_j w_j |v_j|        (points 5, 6).
The code divides by sum_j w_j exp(-a_j), a_j = u + ln2 Es_j, the exact lower end of sum_j w_j (1 + e_j): it is never below 1 - sum_j w_j eta_j, so the bound
is never wider than the line above, and it stays positive where a common score offset of +-120 log2 units makes sum_j w_j eta_j approach 1 in bf16.
o_accumulate: the last two terms times |o_scale|, plus 2 2^-24 (|prev| + |o_scale o|) for the f32 multiply-add, and ulp_T of the accumulated result.

16-bit temporal kernel (csrc/temporal_attn.hip): q and k enter the MFMA as stored (no Q' rounding: Es_j = (d + 8) 2^-24 scale log2e sum_i |q_i| |k_ji|, the 8
covering (s - max) * scale log2e in f32 and exp2); the weights are normalised in f32 BEFORE they are rounded to T (p_j * (1 / sum)), so their sum is no
longer 1 and the middle term acts on |v_j| instead of |v_j - o|; P V is an f32 MFMA sum over F frames: (F + 8) 2^-24 sum_j w_j |v_j|.
Here the rounding of P is charged r = 2 u = 2^-8 (bf16), 2^-11 (f16), the unit roundoff of the type: eta_j = expm1(r + ln2 Es_j).  Half a unit in the last
place is u of a number just below a power of two but 2 u of one just above.  In the flash form u is kept: its single roundings sit beside an Es_j that is an
ABSOLUTE sum over d products and several times larger (the model of tests/attention_cases.py stays below 0.98 of that bound, the ulp_T term included).  A
temporal row of two frames has nothing beside it - one weight near 0.47, rounded down by nearly 2 u, carries the whole error - and correct arithmetic (the
same model) left a bound with u there, at 1.15 x for F = 2 and at 1.02 x for F = 17: the derivation had charged a single rounding half of what it can be.
RoPE: kernel and reference both evaluate x cos -/+ x' sin in f32 and round once to T, but the kernel may contract the sum into an FMA, so a rotated element
may land on the neighbouring T number: Es_j gains scale log2e sum_i (ulp_T(q'_i) |k'_ji| + |q'_i| ulp_T(k'_ji) + ulp_T(q'_i) ulp_T(k'_ji)), q', k' the
reference's rotated, rounded values.

f32 temporal kernel (one thread per query frame, fmaf chains): the same form with u = 2^-24: Es_j = (d + 8) u scale log2e sum_i |q_i| |k_ji|; expf is assumed
good to 4 ulp on an argument that itself carries 2 u |s_j - max| from the scale product and the subtraction, eta_j = expm1(4 u + 2 u |s_j - max| + ln2 Es_j);
nothing is rounded to a 16-bit type, the weights are normalised before use (middle term on |v_j|), P V is a chain of F fmaf: (F + 8) u sum_j w_j |v_j|.
RoPE in f32: three roundings per rotated element on either side, contracted or not: Es_j gains the term above with 3 u (|x cos| + |x' sin|) in place of ulp_T.

The constant in front of these terms is 1, like C_ACC.  A CPU model of the rounding points (tests/attention_cases.py) stays below the bound on every case
(tests/test_attention_cases.py); what the MI355X measured is in profiles/attention_bound_coverage.txt.

Normalisation kernels (csrc/norm.hip, csrc/chan_parts.h).  The bounds are computed in tests/norm_cases.py beside the f64 references and handed to compare() as `bound`;
u = 2^-24 throughout (all arithmetic is f32, whatever the storage type T), the constant is 1, ulp_T(ref) is added for the store (for T = f32 the kernel does not round again
there, but the reference does when it is stored: half of that unit is the reference's own, the other half is slack).
  Statistics (fyc_gn_stats), per {sum, sum sq} entry, the two judged separately:  |s - s_ref| <= L u sum |x|,  |q - q_ref| <= (L + 1) u sum x^2.  L is the longest chain of f32
    additions a term passes through: the rows one thread walks (the 4-row tree has fewer roundings on a term's path than the row-by-row tail) + rpi row lanes + the channels of a
    group.  The + 1 is the rounding of the square and is charged for T = f32 only: the square of a bf16 / f16 number is exact in f32.  The f64 additions of the chunk partials
    cost 2^-53 each.  Integer-valued inputs in [-3, 3] keep every f32 partial an integer below 2^24: the result must be the f64 sum bit for bit.
  fyc_gn_apply: m = s / n, var = q / n - m^2 in f64 (4 2^-53 (q / n + m^2)), then mean_f = (float)m: dm = u |m| + ds / n;  dvar = dq / n + 2 |m| ds / n (zero from exact
    statistics); rstd = rsqrtf((float)var + eps) has the relative error rho = (dvar + u var + u (var + eps)) / (2 (var + eps)) + 2 u - the conversion, the addition, and rsqrtf at
    the 1 ulp (= up to 2 u) of the HIP math API's accuracy table.  o = (x - mean) * rstd * g + b is charged FOUR f32 roundings, one more than the three of a fused form: the
    library is built with -ffp-contract=off (followyourclick_amd/_build.py), so * g + b is a product and a sum (the CPU model runs that order, and the fused one as well):
        |o - o_ref| <= |g| rstd dm + |(x - m) rstd g| (rho + 3 u) + u |o|.
  fyc_gn_apply_cs: sc = rstd g (rho + u), mean_f sc (dm |sc|, the error of sc, and its own rounding: the u |mean sc| term), sf = beta - mean sc (u |sf|), one fused multiply-add:
        |o - o_ref| <= |x sc| (rho + u) + dm |sc| + |m sc| (rho + u) + u |m sc| + u |sf| + u |o|;
    the f64 fold of the channel sums (reduced sums or row-tile partials, 8 lanes and 3 shuffles) is charged n 2^-53 sum |terms|.  With mean / std = 64 the terms |x sc| and
    |m sc| are 64 times the output: that, not the f64 subtraction, is where an ill-conditioned GroupNorm loses its digits.
  SiLU: silu_f(o) = o / (1 + __expf(-o)), __expf = exp2(-o log2e).  E = exp(-o) carries the relative error u |o| of the rounded product (u |o| log2e in log2 units), 0.25 u |o| of
    log2e as an f32 constant (it is off by 0.22 u), 2 u of the instruction (1 ulp); through d silu / dE = -o / (1 + E)^2, plus the addition and the division (u |silu| each) and
    |silu'(o)| times the error of o.
  fyc_layernorm / fyc_row_stats (16 lanes per row, two passes): a lane adds its 8 need values in a chain and 4 shuffles follow, L = 8 need + 4; mean = s / C:
    dm = L u sum |x| / C + u |m|.  q = sum fl(fl(x - mean_f)^2): the common shift dm adds dm^2 per element (sum (x - m) = 0 removes the cross term), each difference and each
    square one rounding, the sum its chain: dvar = dm^2 + (L + 3) u sum (|x - m| + dm)^2 / C + u var; rho and the four roundings of the output as for fyc_gn_apply, one more
    for the positional row.  row_stats: |mean - m| <= dm and |rstd - rstd_ref| <= rstd rho, each plus the f32 ulp of the stored reference, judged separately.
  fyc_softmax_rows: the maximum is exact; x - max is one rounding (u |x - max| on the exponent), expf the 1 ulp (2 u) OCML documents: eta_j = u |x_j - max| + 2 u; the sum is a
    chain of `laps` terms per thread, 6 shuffles and 3 additions; one reciprocal, one product:  |p_j - ref_j| <= p_j (eta_j + sum_k p_k eta_k + (laps + 11) u) + ulp_T(ref_j).
    Masked (causal) columns must be exact zeros.
  fyc_chan_stats_reduce and the fold of fyc_gn_apply_cs: f64 sums of f32 values, n 2^-53 sum |terms|; with integer-valued partials exact.
A torch model of these rounding points (tests/norm_cases.py: f32 tensors combined in the kernel's order) stays inside every bound (tests/test_norm_cases.py); what the MI355X
measured is in profiles/norm_bound_coverage.txt.

Row-panel kernels (csrc/panel_linear.hip, csrc/ff_block.hip).  The bounds are computed in tests/row_panel_cases.py beside the reference of EmuOps(acc=float64) and handed to
compare() as `bound`; u = 2^-24, the constant is 1.  These kernels round INTERMEDIATES to the storage type T, and so does the reference, at the same places.  For such an intermediate
with exact value z the kernel holds z + d before it rounds, |d| <= e, e the f32 error of the kernel's arithmetic up to there.  If no rounding boundary of T (the middle of two
neighbouring T numbers) lies within e of z, both sides store the SAME T number and the stage costs nothing; otherwise the kernel may store the neighbour, and the element is charged
the distance between the T numbers of z - e, z and z + e (one ulp_T unless e exceeds it; row_panel_cases.spread).  The charge goes through the next stage with the absolute values
of that stage's weights.  The last stage is a GEMM and gets ulp_T(ref) + (K + 8) u S as element_bound does, S including bias and residual.
  fyc_panel_linear, GroupNorm on the operand registers (panel_linear.hip:104-115, :131): mean and var = q / cnt - mean^2 in f64 from f64 sums (rel64 = 8 2^-53 (q / cnt + mean^2) /
    (2 (var + eps)) + 64 2^-53 on rstd, the latter for the order of the f64 additions), rstd -> f32 (u), sc = rstd * gamma (u), (float)mean (u), mean * sc (u), sh = beta - mean sc
    (u |sh|), xn = fmaf(x, sc, sh) (u |xn|), then T:
        e = |x sc| (2 u + rel64) + |mean sc| (4 u + rel64) + u |sh| + u |xn|;        out: ulp_T(ref) + (K + 8) u (|xn_T| |W|^T + |bias| + |res|) + charge |W|^T   (:163, :179).
    Without GroupNorm nothing is charged and the bound is element_bound()'s.
  fyc_ff_block, LayerNorm in registers (ff_block.hip:136-156, :187): a lane adds its 160 tokens pair by pair in a fixed order, the two lanes of a row meet, * (1.0f / 320); the sum of
    squares about that mean by fmaf.  These are correctly rounded f32 operations in an order the source fixes (the library is built with -ffp-contract=off), so a simulation in f32
    (row_panel_cases.ff_stats_sim, fmaf emulated exactly) HAS the kernel's mean and variance v, and their error is computed, not bounded: Higham's (n - 1) u sum |x| for a chain of
    160 would put 1.6 % of a large-mean row's elements beside a bf16 boundary.  Left are rsqrtf (1 ulp = 2 u) and the product (u):  e = |(x - mu) / sqrt(v) - xn| + 3 u |xn|.
  FF1 + bias (ff_block.hip:204, :222-223): dv, dg = (320 + 8) u (|xn_T| |W1|^T + |b1|) + charge_xn |W1|^T for value and gate.
  geglu_one (csrc/fyc_common.h): h = v (g Phi_p(g)), Phi_p the degree-7 polynomial in the clamped g.  PHI_ERR = max |Phi_p - Phi| is evaluated in f64 on a dense grid against
    torch.special.erf (row_panel_cases.phi_poly_error; the test repeats it on a finer grid) - it is 1.4e-4, not the 9e-5 the header quotes for x Phi(x).  Its f32 evaluation (xc^2,
    seven fmaf, two products, one fmaf): rnd(g) = |xc| / 2 * 16 u sum |c_i| xc^2i + 3 u.  With DG = 1.13 >= |d/dg (g Phi(g))|:
        e_h = dv |g Phi(g)| + |v| (DG dg + |g| (PHI_ERR + rnd(g))) + DG dv dg + 3 u |h|;
        out: ulp_T(ref) + (320 + 1280 + 8) u (|x| |Wp|^T + |h_T| |W2'|^T + |b_out| + |res|) + charge_h |W2'|^T        (one f32 chain over projection and FF2: :173, :241, :331).
  chan_parts of fyc_ff_block (:339-378), against the f64 sums of the values AS STORED by the same launch: L u sum |x| and (L + 1) u sum x^2 with L = 22 + 6 (a thread adds at most
    22 rows, then the 6 row slices are added), plus the f32 spacing of the reference as stored; an integer-valued output gives the f64 sums bit for bit.
  The shares of charged elements are a condition on the INPUTS, asserted from the reference alone (tests/test_row_panel_cases.py): at most 1 % of a row's xn and 25 % of a row's
    hidden elements.  The recipes of row_panel_cases say what that takes - f16 operands kept away from zero, FF1 rows of about 8 weights, gates mostly positive, and in f16 six
    hidden units per chunk with a value path - because (K + 8) u S of a dense K = 320 row is of the size of the f16 spacing.
The torch model of these rounding points stays inside every bound and every declared defect leaves it (tests/test_row_panel_cases.py); what the MI355X measured is in
profiles/row_panel_bound_coverage.txt.
  fyc_temporal_block (csrc/temporal_block.hip, the LDS-tile kernel; csrc/temporal_block_rr.hip, the register-resident one).  q, k, v are rounded to T by both kernels and by the
    reference; each element is charged by the boundary test above with
      rr (:107-137, :175, :186): xn as for fyc_ff_block (row_panel_cases.tb_stats_sim has this kernel's order: 80 tokens per lane in pairs, four lanes per row), then
        e = (320 + 8) u (|xn_T| |W|^T + |bias + pe|) + charge_xn |W|^T;
      LDS-tile (:69-84, :166): the raw tokens enter the MFMA, the LayerNorm is folded: rs (acc - mu colsum) + bias + pe with mu and the variance q / C - mu^2 of the simulated f32
        chain (four threads per row, 80 tokens each) and rs within 2 u of 1 / sqrt:  e = |that value - the f64 one| + rs (321 u |x| |W'|^T + 2 u |mu colsum|) + 6 u (the terms).
    The attention core is softmax_bound_terms(kind="temporal") on the reference's rounded q, k, v with dq, dk, dv = those charges: the rounding of P is charged there
    unconditionally (r per weight; the rr kernel rounds the exponentials before it normalises them, :247-249, the LDS-tile kernel after, :219 - the emulator now does each as its
    kernel does), and the reference's own rounded weights are within r sum w |v| of the exact ones.  The attention output is rounded to T on both sides: charged by the boundary
    test with e = rest + r sum_j w_j |v_j|, which in practice charges every element.  Output projection over 8 heads x 64 k-slots, bias and residual:
        out: ulp_T(ref) + (512 + 8) u (|x| + |O_T| |Wo|^T + |b_out|) + charge_O |Wo|^T.

The other epilogues of fyc_gemm (csrc/gemm_kernel.h: GEGLU, head split, LINEAR with an activation, the folded LayerNorm in each of them, dual-source K, the unsplit frame-axis
convolution).  The bounds are computed in tests/gemm_cases.py::analysis beside the reference of EmuOps(acc=float64) - exact-erf GELU, the exact fold, x sigmoid(1.702 x); never a copy
of the kernel's polynomial - and handed to compare() as `bound` with lines=True; u = 2^-24, the constant is 1, ulp_T(ref) is added for the store, no element is exempt.
  Pre-activation: pre = acc + bias with acc an f32 sum of K products (of two sources, of three gathered taps: the operand's indexing does not change the count):
        E = (K + 8) u S,  S = |a| |W|^T + |bias|,  as element_bound has it.
  Fold: pre = rs (acc - mu cs) + bias.  The narrow and the LDS-staged forms (the LINEAR, GEGLU and HEADS branches of gemm_epilogue) round mu cs, the difference, the product with rs and the sum with the bias; the
    pack-first forms (epilogue_linear_packed, epilogue_heads_packed, epilogue_geglu_packed) round nm = -rs mu, the inner fma(nm, cs, bias) and the outer fma(acc, rs, .), the head split also rs scale and scale * (.): at most five
    roundings, each on a partial sum no larger than S = rs (|a| |W|^T + |mu cs|) + |bias|, and the K roundings of acc come through rs: E = (K + 8) u S again, with this S.  With
    |mean| / std = 4 the term |mu cs| is several times the output: the cancellation is in S, not assumed away.  Stored {mean, rstd} pairs are the same f32 numbers on both sides.
    ln_nparts (ln_row): n - 1 f32 additions per sum, inv = 1.0f / K (u) and one product each (u): dmu = (n - 1) u sum |s_i| / K + 2 u |mu|;  dvar = (n + 1) u q / K +
    2 |mu| dmu + u mu^2, the subtraction and + eps and rsqrtf at its documented 1 ulp charged as norm_cases.norm_rho charges rstd: drs = rs rho.  These are distances from the
    EXACT statistics of the f32 partials; the reference (EmuOps.gemm) evaluates them in f32 too, in torch's order, and its own distance from the exact ones is computed and added.
        E += drs |acc - mu cs| + rs dmu |cs|.
  LINEAR (lnfold, dualk, t3) and HEADS: out = (pre + res) scale: the residual and the scale are two more of the K + 8 roundings, ulp_T(ref) + (K + 8) u |scale| (S + |res|) (+ |scale|
    times the ln_nparts term).  The head split only moves elements: each segment is a window of its own with this bound.
  GEGLU, 16-bit wide forms (geglu_pair, csrc/fyc_common.h:221): h = v (g Phi_p(g)), exactly the gate of fyc_ff_block: row_panel_cases.PHI_ERR, phi_rounding and DG are reused,
        e = dv |g Phi(g)| + |v| (DG dg + |g| (PHI_ERR + rnd(g))) + DG dv dg + 3 u |h|,  dv, dg = E of the value and the gate column.
  gelu_erf_f (fyc_common.h:190; the narrow GEGLU, f32, and act = 1): GELU_AS_ERR = max |gelu_erf_f - x Phi(x)| of the Abramowitz-Stegun form itself, evaluated in f64 with the
    source's f32 constants on a grid of 2^21 points over |x| <= 12 against torch.special.erf: 2.12e-7 (beyond 12 both sides are x or 0).  Its f32 evaluation is a running first-order
    bound that follows the source operation by operation (gemm_cases.gelu_as): z = |g| c (u), fma(p, z, 1) (u), rcp (1 ulp = 2 u), four Horner fma (u each), poly t (u), z z (u),
    __expf = exp2(x log2e) - the product (u |x|), log2e as an f32 constant (0.25 u |x|), the instruction (2 u) -, the product with it (u), 2 - e (u), the last product (u).
        GEGLU: e = dv |gelu(g)| + |v| (DG dg + GELU_AS_ERR + rnd_as(g)) + DG dv dg + u |h|;        act = 1: e_y = DG E + GELU_AS_ERR + rnd_as(pre).
  Quick-GELU (activate): y = x / (1 + __expf(-1.702f x)).  a = 1.702 x; exp(-a) is off by r = |a| (2.25 u + |1.702f / 1.702 - 1|) + 2 u relative - the rounded product, the
    product and the constant inside __expf, the kernel's f32 constant against the reference's 1.702, the instruction - and moves y by |x| E / (1 + E)^2 r; the addition and the
    division (correctly rounded) are u |y| each.  Slope DQ = 1.10 >= |d/dx x sigmoid(1.702 x)| (1.0998 on a grid, as DG = 1.13 >= 1.1290):  e_y = DQ E + that.
  After the activation: out = (y + res) scale, two roundings:  ulp_T(ref) + |scale| (e_y + 2 u (|y| + |res|)).
  A condition on the INPUTS of the GEGLU cases: gates centred on +1.5.  In f16 the polynomial's 1.4e-4 on Phi alone puts a row or column of mostly negative gates at the line
    tolerance of 5e-4 (gemm_cases.epilogue_operands has the arithmetic); the per-element bound holds for either sign and 7 % of the gates stay negative.
A torch model of every form stays inside these bounds, every declared single-site defect leaves them or trips the guard, and the slopes and approximation errors are evaluated on
grids (tests/test_gemm_epilogue_cases.py); what the MI355X measured is part 4 of profiles/gemm_epilogue_coverage.txt.
"""
import math
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


U = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12, "f32": 2.0 ** -24}      # the u of the softmax bounds (module docstring)
R = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}      # the unit roundoff r: what the rounding of P is charged in the temporal form
LOG2E, LN2 = 1.4426950408889634, math.log(2.0)
# row / column labels of an attention output for compare()'s messages: rows are (batch, query) or (clip, frame, pixel), columns (head, channel)
Labels = namedtuple("Labels", ["row", "col"])


def softmax_bound_terms(q, k, v, *, scale, dtype, kind, dq=None, dk=None, dv=None):
    """One (batch, head), or a few with leading dimensions: q [n_q][d], k [n_k][d], v [n_k][d] as f64 -> (o, rest, w): the f64 reference output [n_q][d], the bound WITHOUT its ulp_T(ref)
    term (the caller rounds o into its buffer and adds the ulp of what it stored) and the reference weights [n_q][n_k].  kind: "flash" or "temporal"
    (16-bit or f32 by dtype); dq, dk: per-element uncertainty of the rotated q and k (RoPE), same shapes; dv: per-element uncertainty of v, charged as w @ dv with the kernel's own weights (at most
    (w_j + w_j eta_j) / den).  The middle term is O(n_q n_k d): call per head."""
    assert q.dtype == k.dtype == v.dtype == torch.float64 and kind in ("flash", "temporal")
    d, n_k, u, f32 = q.shape[-1], k.shape[-2], U[dtype], 2.0 ** -24
    r = u if kind == "flash" else R[dtype]      # what one rounding to T is charged (module docstring)
    kt = k.transpose(-1, -2)
    s = (q @ kt) * scale
    w = torch.softmax(s, dim=-1)
    o = w @ v
    Es = ((r if kind == "flash" else 0.0) + (d + 8) * f32) * scale * LOG2E * (q.abs() @ kt.abs())
    if dq is not None:
        Es = Es + scale * LOG2E * (dq.abs() @ kt.abs() + q.abs() @ dk.abs().transpose(-1, -2) + dq.abs() @ dk.abs().transpose(-1, -2))
    arg = r + LN2 * Es if dtype != "f32" else 4 * u + 2 * u * (s - s.max(dim=-1, keepdim=True).values).abs() + LN2 * Es
    we = w * torch.expm1(arg)
    dev = (v[..., None, :, :] - o[..., :, None, :]).abs() if kind == "flash" else v.abs()[..., None, :, :]
    den = (w * torch.exp(-arg)).sum(dim=-1, keepdim=True)      # sum_j w_j (1 + e_j) >= sum_j w_j exp(-a_j) (>= 1 - sum_j w_j eta_j, and never 0)
    rest = (we[..., None] * dev).sum(dim=-2) / den + (n_k + 8) * f32 * (w @ v.abs())
    if dv is not None:
        rest = rest + ((w + we) @ dv.abs()) / den
    return o, rest, w


def _where(i, j, tile, prefix=""):
    if isinstance(tile, Labels):
        return f"{prefix}row {i} ({tile.row(i)}), column {j} ({tile.col(j)})"
    bm, bn = tile
    return (f"{prefix}row {i}, column {j} (row tile {i // bm} of {bm} rows, row {i % bm} in it; column tile {j // bn} of {bn} columns, column {j % bn} in it; "
            f"16-row pass {i % bm // 16}, lane column {j % 16})")


def _bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def compare(got, ref, *, dtype, bound_terms=None, guard=None, tag, bound=None, rtol=None, labels=None, lines=False):
    """With `bound` ([rows][columns] f64, a precomputed per-element bound: the softmax bounds of the module docstring), `rtol` (the global tolerance to
    assert) and `labels` (a Labels): (a), (b), (d), (e) below.  (c) is skipped: a single attention row whose arithmetic is right can sit at several times
    the project's global tolerance (one rounding of a dominant probability moves the whole row), which is exactly why the bound is per element.
    `lines=True` runs (c) in this form as well, at `rtol` (the row-panel kernels: a row or a column is a dot product of hundreds of terms, none of which dominates).

    got, ref: [rows][columns], the kernel's output window and the reference from EmuOps(acc=torch.float64), both in the storage type `dtype`
    ("bf16" / "f16" / "f32").  Asserts, in this order: (a) finite everywhere, (b) global relative L2 <= RTOL[dtype], (c) relative L2 of every row and
    of every column <= RTOL[dtype] (rows / columns whose reference norm is below the norm of their per-element bounds are left to (d)),
    (d) every element within element_bound(), (e) everything outside guard.mask bit-identical.  No element is exempt from (d)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    if bound is not None:
        assert bound_terms is None and rtol is not None and labels is not None
        assert g.dim() == 2 and g.shape == r.shape == tuple(bound.shape), (tag, g.shape, r.shape, tuple(bound.shape))
        tile, form = labels, "its precomputed bound"
    else:
        assert g.dim() == 2 and g.shape == r.shape == tuple(bound_terms.S.shape), (tag, g.shape, r.shape, tuple(bound_terms.S.shape))
        tile, rtol, form = bound_terms.tile, RTOL[dtype], f"ulp + {C_ACC:g} (K + 8) 2^-24 S"
    fig = last_figures
    fig.clear()
    fig.update(tag=tag, dtype=dtype)
    # (a)
    nonfin = (~torch.isfinite(g)).nonzero()
    assert nonfin.numel() == 0, f"{tag}: {nonfin.shape[0]} non-finite values, first at {_where(*nonfin[0].tolist(), tile)}"
    diff = g - r
    bound = element_bound(r, dtype, bound_terms) if bound is None else bound.detach().cpu().double()
    ratio = diff.abs() / bound
    worst = int(ratio.argmax())
    wi, wj = divmod(worst, g.shape[1])
    # (b)
    rel = (diff.norm() / (r.norm() + 1e-300)).item()
    fig.update(global_rel=rel, elem_ratio=ratio.max().item())
    assert rel <= rtol, f"{tag}: global rel-L2 {rel:.3e} > {rtol:.1e}; worst element {ratio.max().item():.3g} x its bound at {_where(wi, wj, tile)}"
    # (c)
    for axis, what in ((1, "row"), (0, "column")) if (bound_terms is not None or lines) else ():
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
        raise AssertionError(f"{tag}: {over.shape[0]} of {g.numel()} elements outside |got - ref| <= {form}; first: got {g[i, j].item():.8g}, "
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
