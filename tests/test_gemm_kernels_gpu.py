"""The dense GEMM entry points (ia_gemm_bf16, ia_gemm_bf16_qscale) through the C ABI against the fp64 reference of
tests/gemm_reference.py, ELEMENT BY ELEMENT, for every form gemm_core's switch dispatches and every output the form has.

Two kinds of operands per case: `exact_operands`, on which every linear output is a number its type holds exactly in any summation order
-- there got == reference everywhere, so a product left out, doubled or taken from a neighbouring row, or a pad column read past a ragged
K, shows as a whole unit -- and ordinary ones (randn), held to the derived per-element bars of gemm_reference.bars (checked on the host
against a CPU model of the kernels' rounding by tests/test_gemm_reference_host.py, never fitted to a GPU result).  The GELU forms use
their bar on both: nothing there is exact, but on the exact operands the pre-activations are known bf16 numbers.

Every call runs on PITCHED buffers: lda / ldb = the row length + 8 rounded up to a multiple of 8 with bf16 NaN in the pad columns and
in 8 rows behind the operand; C, C2 and aux with ldc = ldaux = N + 4, a sentinel (NaN for aux) in the pad columns and in 64 guard rows
behind the last row (IA_EPI_DGELU_COLSUM needs ldc == N: there only the guard rows).  Pads, guard rows, the inputs and the bytes behind
the stated workspace size have to come back bit-unchanged, and a second call on unpitched buffers (the smallest legal pitches) has to be
torch.equal to the pitched one.  A NaN in an output is a pad that was read into a stored value.

Each case ASSERTS the path it is meant for from what the library exports (ia_gemm_fwd_rows_filters / ia_gemm_dgrad_rows_filters /
ia_gemm_wgrad_rows_filters tell the 256-wide kernels from T128, ia_gemm_workspace_bytes gives the planned split count): a change of
make_plan turns a silently re-routed case into a failure.  Every comparison prints max error / bar (`-s` shows them).

Out of scope: the shifted views and channel groups of ia_gemm_view (tests/test_conv_kernels_gpu.py holds them to fp64 element by element
through the convolution entry points) and the filtered entry points (pinned bit-for-bit to the dense call by their own files).
"""
import pytest
import torch

import gemm_reference as R

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD = 64
SENT = 768.0           # sentinel of the outputs' pad columns and guard rows (exact in bf16)
NAN = float("nan")
WS_TAIL = 256          # bytes behind the stated workspace size that have to stay untouched
RATIOS = {}

T128_SHAPES = [(1, 4, 8), (77, 132, 72), (128, 64, 64), (129, 256, 200), (300, 392, 1024), (300, 132, 128)]
T128_SHAPES_N8 = [(1, 64, 8), (77, 256, 72), (128, 64, 64), (129, 256, 200), (300, 392, 1024), (300, 64, 128)]      # ia_colsum: N a multiple of 8
T128_SHAPES_Q = [(77, 132, 72), (129, 256, 200), (300, 392, 1024), (128, 256, 8), (1, 132, 64), (300, 132, 128)]    # N >= 128: one scaled 128-block
T128_SHAPES_TN = [(1, 4, 1), (77, 132, 40), (128, 64, 300), (129, 256, 333), (300, 392, 40), (300, 132, 333)]
WIDE_K = [8, 64, 72, 128, 192, 1024]
WIDE_EDGES = [(5120, 2048, 192), (5100, 2184, 192)]


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def pools(gpu):
    """every draw of the module, once: [5120, 1024] x [1024, 4096] for the bf16 forms, two deep pools for the split-K shapes"""
    g = torch.Generator(device="cuda").manual_seed(6021)
    mk = lambda M, N, K: (R.exact_pool(g, M, N, K), R.normal_pool(g, M, N, K))
    return {"flat": mk(5120, 4096, 1024), "wgrad": mk(1024, 1024, 7168), "deep": mk(128, 576, 70000)}


def r8(n):
    return (n + 7) & ~7


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else torch.uint8)


def padded(x, ld, fill, guard):
    """x [rows, cols] inside a buffer [rows + guard, ld] of `fill`"""
    buf = torch.full((x.shape[0] + guard, ld), fill, dtype=x.dtype, device=x.device)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf


def vec(x, n, fill):
    buf = torch.full((n + GUARD,), fill, dtype=F32, device="cuda")
    if x is not None:
        buf[:n] = x
    return buf


def same_outside(what, before, after, rows, cols=None):
    """everything but the real elements [:rows, :cols] (or [:rows] of a vector) has to come back bit-unchanged"""
    a, b = bits(after).clone(), bits(before).clone()
    if cols is None:
        a[:rows] = 0; b[:rows] = 0
    else:
        a[:rows, :cols] = 0; b[:rows, :cols] = 0
    assert torch.equal(a, b), what + ": pad columns or guard rows were written"


def is_wide(lib, form, M, N, K):
    if form.f32:
        return bool(lib.ia_gemm_wgrad_rows_filters(M, N, K))
    return bool(lib.ia_gemm_dgrad_rows_filters(M, N, K) if form.bks else lib.ia_gemm_fwd_rows_filters(M, N, K))


def planned_splits(lib, M, N, K):
    b = lib.ia_gemm_workspace_bytes(M, N, K, 1)
    assert b % (4 * M * (N + 1)) == 0
    return b // (4 * M * (N + 1)) if b else 1


def run(lib, form, ops, M, N, K, pitch):
    """one call of `form` on freshly built buffers; returns the real elements of every output"""
    from item_alignment_amd import _lib
    cs = form.epi == R.EPI_DGELU_COLSUM
    a = ops["A"].t() if form.aks else ops["A"]
    b = ops["B"] if form.bks else ops["B"].t()
    extra = 8 if pitch else 0
    A = padded(a.to(BF16), r8(a.shape[1] + extra), NAN, 8)
    B = padded(b.to(BF16), r8(b.shape[1] + extra), NAN, 8)
    ldc = N + 4 if pitch and not cs else N
    ldaux = N + 4 if pitch else N
    cdt = F32 if form.f32 else BF16
    C = padded(ops["prior"].to(cdt) if form.acc else torch.full((M, N), SENT, dtype=cdt, device="cuda"), ldc, SENT, GUARD)
    aux = padded(ops["aux"].to(BF16), ldaux, NAN, GUARD) if ops["aux"] is not None else None
    bias = ops["bias"].to(F32).contiguous() if ops["bias"] is not None else None
    C2, c2_rows = None, 0
    if form.epi == R.EPI_BIAS_GELU:
        C2 = padded(torch.full((M, N), SENT, dtype=BF16, device="cuda"), ldc, SENT, GUARD)
    elif form.c2:
        c2_rows = N if cs else M
        C2 = vec(ops["prior2"], c2_rows, SENT)
    wsb = 16
    if form.f32:
        wsb = max(wsb, lib.ia_gemm_workspace_bytes(M, N, K, 1))
        if form.c2:
            wsb = max(wsb, lib.ia_colsum_workspace_bytes(K, M))
    if cs:
        wsb = max(wsb, lib.ia_gemm_colsum_workspace_bytes(M, N))
    ws = torch.full((wsb + WS_TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    before = {k: t.clone() for k, t in (("A", A), ("B", B), ("C", C), ("C2", C2), ("aux", aux), ("bias", bias)) if t is not None}
    p = lambda t: None if t is None else t.data_ptr()
    if form.q:
        rc = lib.ia_gemm_bf16_qscale(p(A), A.shape[1], p(B), B.shape[1], p(C), ldc, M, N, K, p(bias), ops["qcols"], ops["qscale"], _lib.stream_ptr())
    else:
        rc = lib.ia_gemm_bf16(p(A), int(form.aks), A.shape[1], p(B), int(form.bks), B.shape[1], p(C), int(form.f32), ldc, M, N, K, form.epi, p(bias),
                              p(aux), ldaux, p(C2), int(form.acc), p(ws), wsb, _lib.stream_ptr())
    _lib.check(rc, form.name)
    torch.cuda.synchronize()
    what = "%s %dx%dx%d %s" % (form.name, M, N, K, "pitched" if pitch else "unpitched")
    for k, t in (("A", A), ("B", B), ("aux", aux), ("bias", bias)):
        if t is not None:
            assert torch.equal(bits(before[k]), bits(t)), what + ": input " + k + " was written"
    assert bool((ws[wsb:] == 0x5A).all()), what + ": the workspace was written past its stated size"
    same_outside(what + " C", before["C"], C, M, N)
    out = {"C": C[:M, :N].clone()}
    if form.epi == R.EPI_BIAS_GELU:
        same_outside(what + " C2", before["C2"], C2, M, N)
        out["C2"] = C2[:M, :N].clone()
    elif form.c2:
        same_outside(what + " C2", before["C2"], C2, c2_rows)
        out["C2"] = C2[:c2_rows].clone()
    return out


def check(lib, pool, form, M, N, K, wide, qcols=0, kinds=("exact", "normal"), min_splits=None, max_splits=None):
    """`form` at M x N x K on both kinds of operands: the path, pitched == unpitched, every output against fp64.  Returns the pitched
    outputs per kind."""
    assert is_wide(lib, form, M, N, K) == wide, (form.name, M, N, K, "planned for the other tile configuration")
    splits = planned_splits(lib, M, N, K) if form.f32 and form.epi == R.EPI_NONE else 1
    if min_splits is not None:
        assert min_splits <= planned_splits(lib, M, N, K) <= max_splits, (form.name, M, N, K, planned_splits(lib, M, N, K))
    res = {}
    for kind in kinds:
        exact = kind == "exact"
        ops = (R.exact_operands if exact else R.normal_operands)(pool[0 if exact else 1], form, M, N, K, "cuda", qcols)
        got = run(lib, form, ops, M, N, K, True)
        plain = run(lib, form, ops, M, N, K, False)
        bar = R.bars_of(form, ops, splits, exact=exact, stored_colsum=not wide)
        for key, want in ops["ref"].items():
            where = "%s %s %dx%dx%d %s operands (%s, %d k-slabs planned)" % (form.name, key, M, N, K, kind, "256-wide" if wide else "T128", splits)
            assert torch.equal(got[key], plain[key]), where + ": pitched and unpitched calls differ: " + str(
                R.first_bad(got[key].to(F64), plain[key].to(F64), torch.zeros_like(want)))
            g64 = got[key].to(F64)
            ratio = R.worst_ratio(g64, want, bar[key])
            tag = (form.name + (" exact" if exact else ""), key)
            if exact and form.epi not in R.GELU:
                assert float(bar[key].max()) == 0.0
            else:
                RATIOS[tag] = max(RATIOS.get(tag, 0.0), ratio)
                print("%-90s worst error / bar %.3f" % (where, ratio))
            bad = R.first_bad(g64, want, bar[key])
            assert bad is None, where + ": " + bad
        res[kind] = got
    return res


def report(forms):
    for (name, key), r in sorted(RATIOS.items()):
        if any(name == f.name or name == f.name + " exact" for f in forms):
            print("worst so far  %-28s %-2s  error / bar %.3f" % (name, key, r))


# ------------------------------------------------------------------------------------------------------------------ T128
@pytest.mark.parametrize("form", R.NT_BF16 + R.NN_BF16 + R.NT_F32, ids=lambda f: f.name)
def test_t128_edges(lib, pools, form):
    """T128 (asserted): every M edge {1, 77, 128, 129, 300}, N edge {4, 64, 132, 256, 392} and K edge {8, 64, 72, 128, 200, 1024} at least
    once per form.  N = 132 is a multiple of 4 and not of 8: the path only T128 serves.  The column-sum form takes N from the multiples
    of 8 (its second stage, ia_colsum, accepts no other), the scaled-column form N >= 128."""
    shapes = T128_SHAPES_N8 if form.epi == R.EPI_DGELU_COLSUM else T128_SHAPES_Q if form.q else T128_SHAPES
    for M, N, K in shapes:
        check(lib, pools["flat"], form, M, N, K, False, qcols=(N // 128 + 1) // 2 * 128 if form.q else 0)
    report([form])


@pytest.mark.parametrize("form", R.TN_F32, ids=lambda f: f.name)
def test_t128_weight_gradient_form_edges(lib, pools, form):
    """k-strided A and B, fp32 output, T128 (asserted), K in {1, 40, 300, 333}: with and without the row sums, with and without
    `accumulate` onto a random prior.
    Found here: with an odd M the window over the k-strided A ended in the middle of a dword, the buffer range check dropped that dword,
    and the k = K-1 product of row M-1 (and A[K-1][M-1] of the row sums) was missing -- at 1 x 4 x 1 the whole output was 0.  gemm_core
    now ends the window behind that dword."""
    for M, N, K in T128_SHAPES_TN:
        check(lib, pools["flat"], form, M, N, K, False)
    report([form])


@pytest.mark.parametrize("form", R.TN_F32, ids=lambda f: f.name)
@pytest.mark.parametrize("M,N,K,lo,hi", [(64, 576, 5000, 2, 16), (128, 128, 70000, 17, 1 << 20)])
def test_t128_split_k_reaches_both_reduce_kernels(lib, pools, form, M, N, K, lo, hi):
    """splitk_reduce_kernel (up to 16 k-slabs) and splitk_reduce_deep_kernel (more), the planned count asserted from the workspace size;
    each with the row-sum partials the reduce kernels fold, and with `accumulate`."""
    check(lib, pools["deep"], form, M, N, K, False, min_splits=lo, max_splits=hi)
    report([form])


# ------------------------------------------------------------------------------------------------------------------ T256W, bf16 output
@pytest.mark.parametrize("form", [f for f in R.NT_BF16 + R.NN_BF16 if not f.q], ids=lambda f: f.name)
def test_t256w_bf16_edges(lib, pools, form):
    """256-wide (asserted).  5100 x 2048 is 20 x 8 = 160 tiles, the fewest make_plan gives the kernel, the last tile row clipped to 236
    rows; K = 8 (less than a k-tile), 64 (one), 72 (ragged), 128 (two), 192 (odd count), 1024 for the plain, bias and bias + GELU forms,
    K in {72, 192} for the others; 5120 (no clipped row) and N = 2184 (an edge n-tile of 136 columns) at K = 192."""
    every_k = form.name in ("nt", "nt+bias", "nt+bias_gelu")
    for M, N, K in [(5100, 2048, K) for K in (WIDE_K if every_k else (72, 192))] + WIDE_EDGES:
        check(lib, pools["flat"], form, M, N, K, True)
    report([form])


def test_t256w_scaled_columns_where_the_two_epilogue_layouts_meet(lib, pools):
    """qcols = 1024 of N = 3072 at M = 5100 (no multiple of 128: the rows behind the last whole 128-row part leave through the row-layout
    epilogue, (acc + bias) * scale, the others through the accumulator-layout one, acc * scale + bias * scale) and at M = 5120."""
    form = R.FORMS["nt+bias,qcols"]
    for M, N, K in [(5100, 3072, 72), (5100, 3072, 192), (5120, 3072, 192)]:
        check(lib, pools["flat"], form, M, N, K, True, qcols=1024)
    report([form])


@pytest.mark.parametrize("M,N,K", [(5100, 4096, 128), (5100, 4096, 320), (5120, 4096, 128)])
def test_more_tiles_than_workgroups_lookahead_and_draining(lib, pools, monkeypatch, M, N, K):
    """320 tiles on 256 workgroups: the plain NT form under IA_GEMM_LA=1 (the look-ahead kernel) and =0 (t256w's persistent loop), bit-identical
    to each other and both inside the fp64 checks."""
    form = R.FORMS["nt"]
    assert ((M + 255) // 256) * ((N + 255) // 256) > 256
    monkeypatch.setenv("IA_GEMM_LA", "1")
    la = check(lib, pools["flat"], form, M, N, K, True)
    monkeypatch.setenv("IA_GEMM_LA", "0")
    dr = check(lib, pools["flat"], form, M, N, K, True)
    for kind in la:
        assert torch.equal(la[kind]["C"], dr[kind]["C"]), (kind, "the look-ahead kernel and the draining one differ")
    report([form])


@pytest.mark.parametrize("name", ["nt+bias_add", "nn+add"])
def test_more_tiles_than_workgroups_epilogue_second_round(lib, pools, name):
    """one epilogue form of each family at 5100 x 4096 x 192: the persistent loop's second round behind a fused epilogue"""
    check(lib, pools["flat"], R.FORMS[name], 5100, 4096, 192, True)
    report([R.FORMS[name]])


# ------------------------------------------------------------------------------------------------------------------ T256W, fp32 output
@pytest.mark.parametrize("name,M,N,K", [(f.name, 1024, 1024, K) for K in (5120, 5160) for f in R.TN_F32] +
                         [("tn_f32", 768, 1024, 7168), ("tn_f32+rowsum", 768, 1024, 7168)])
def test_t256w_weight_gradient_split_k(lib, pools, name, M, N, K):
    """the weight-gradient form on the 256-wide kernel (asserted) under a split k (asserted > 1), whole and ragged last k-tile; with
    `accumulate`, and with C2: the stand-alone column-sum pass that reuses the workspace after the reduce"""
    check(lib, pools["wgrad"], R.FORMS[name], M, N, K, True, min_splits=2, max_splits=32)
    report([R.FORMS[name]])


@pytest.mark.parametrize("form", R.NT_F32, ids=lambda f: f.name)
def test_t256w_fp32_nt_bias_is_not_cut(lib, pools, form):
    """NT with fp32 output at 1024 x 1024 x 5120: planned 256-wide with a split (both asserted).  The plain form is cut; IA_EPI_BIAS must
    not be -- a bias added once per k-slab shows on the exact operands as whole units (gemm_core recalls 2-8 x the bias)."""
    check(lib, pools["wgrad"], form, 1024, 1024, 5120, True, min_splits=2, max_splits=32)
    report([form])
