"""ia_gemm_fwd_slabs / ia_gemm_dgrad_slabs: the row-filtered GEMMs in 8-row slabs against the unfiltered call on the same inputs, element
for element, and against fp64.

Every instantiation the slab form has: forward EPI_NONE, EPI_BIAS with scaled (q) columns, EPI_BIAS_GELU with both outputs; data gradient
EPI_NONE and EPI_ADD with W k-strided and transposed; and the look-ahead kernel's slab form (plain, both operands k-contiguous, more
tiles than workgroups).

Shapes.  The filter lives in the 256-wide kernels, which a bf16-output call reaches from 160 tiles of 256 x 256 on
(ia_gemm_fwd_rows_filters / ia_gemm_dgrad_rows_filters; smaller calls run every row through the 128-wide kernel whatever the mask says).
So the shapes come in two sets, and every check runs on both:
  * SMALL: M in {264, 765 = 3 x 255 (the last slab holds 5 rows), 1032} x N in {256, 384, 3072 with 1024 scaled columns} x K in
    {64, 192, 1024} -- below 160 tiles: these pin that a call the kernel does not serve still honours the contract (it runs every row,
    so its dead slabs hold the unfiltered values where the fill is on, and are written where it is off);
  * BIG, the smallest that reach each path of the slab kernels (asserted): M = 5100 = 20 x 255 (20 M-tiles when dense; the last slab
    holds 4 rows; 5100 = 39 x 128 + 108, so the scaled columns meet the guarded one-tile launch) and M = 5120 (a multiple of 128: no such
    launch, the last slab whole), N = 2048 (160 tiles), N = 2184 (an edge n-tile whose second wave holds 8 columns), N = 3072 with 1024
    scaled columns, N = 4096 (320 tiles on 256 workgroups: the look-ahead kernel, K = 128 and 320), K in {64 (prologue only), 192 (odd
    k-tile count), 1024}.
Row patterns: tests/slab_masks.py (every row, none, one row, every other slab, only the partial last slab, fewer than / exactly / more
than 32 live slabs, tiles that leave a wave without a slab, drawn lengths).

Checks: rows of live slabs torch.equal to the unfiltered call (both outputs of the GELU form); dead slabs zeros with the fill on and the
sentinel left in place with it off; NaN (forward) / 1e4 (data gradient, whose contract wants zeros in dead rows of live slabs) in the
input rows of dead slabs change nothing; fp64 error of the live rows below 2e-3 of the largest reference element (the bound of
tests/test_gemm_wgrad_blocks_gpu.py) for the linear forms on operands whose outputs bf16 holds exactly, and below the 2e-2 of
tests/test_kernels_gpu.py on normal operands, the GELU form included (test_live_rows_against_fp64 says why two runs)."""
import numpy as np
import pytest
import torch

from slab_masks import expected_list, named_masks, slab_dilate

pytestmark = pytest.mark.gpu

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_ADD = 0, 1, 2, 3
SENTINEL = 768.0      # (exact in bf16)
SMALL = [(M, N, K) for M in (264, 765, 1032) for N in (256, 384, 3072) for K in (64, 192, 1024)]
BIG = [(5100, 2048, 64), (5100, 2048, 192), (5100, 2048, 1024), (5100, 2184, 192), (5120, 2048, 192)]
BIG_Q = [(5100, 3072, 64), (5100, 3072, 1024), (5120, 3072, 192)]
BIG_LA = [(5100, 4096, 128), (5100, 4096, 320), (5120, 4096, 128)]


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.fixture(scope="module")
def operands(gpu):
    g = torch.Generator(device="cpu").manual_seed(8642)
    m, n, k = 5120, 4096, 1024
    # "exact": operands on which every output is a number bf16 holds exactly -- x and w in {-1, 0, 1} (zero half of the time: a sum of
    # 1024 products has a standard deviation of 16 and stays far inside +-200), aux and bias whole numbers in -3 .. 3, the column scale
    # 1/4 -- so the fp32 sums are exact whatever their order, the bf16 store rounds nothing, and what is left against fp64 is the
    # arithmetic alone: a product left out, added twice or taken from a wrong row shows as a whole unit
    tern = lambda *shape: (torch.randint(-1, 2, shape, generator=g) * torch.randint(0, 2, shape, generator=g)).float()
    exact = {"x": tern(m, k).to(gpu).to(torch.bfloat16), "w": tern(n, k).to(gpu).to(torch.bfloat16),
             "aux": torch.randint(-3, 4, (m, n), generator=g).float().to(gpu).to(torch.bfloat16),
             "bias": torch.randint(-3, 4, (n,), generator=g).float().to(gpu), "col_scale": 0.25}
    return {"x": torch.randn((m, k), generator=g).to(gpu).to(torch.bfloat16),
            "w": (torch.randn((n, k), generator=g) * 0.4).to(gpu).to(torch.bfloat16),
            "aux": torch.randn((m, n), generator=g).to(gpu).to(torch.bfloat16),
            "bias": torch.randn(n, generator=g).to(gpu), "exact": exact}


def masks_on(gpu, M):
    for name, live_np in named_masks(M).items():
        yield name, live_np, torch.from_numpy(live_np).to(gpu), torch.from_numpy(slab_dilate(live_np)).to(gpu).bool()


def test_row_slabs_kernel_matches_host(gpu):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    rs = np.random.RandomState(5)
    patterns = [m for M in (264, 765, 5100) for m in named_masks(M).values()]
    patterns += [(rs.rand(130560) < 0.01).astype(np.uint8), (rs.rand(130560) < 0.6).astype(np.uint8), np.ones(33, np.uint8), np.zeros(1, np.uint8)]
    for live in patterns:
        for off in (0, 3):                 # an unaligned row_live pointer too
            buf = torch.zeros(len(live) + off, dtype=torch.uint8)
            buf[off:] = torch.from_numpy(live)
            got = ops.row_slabs(buf.to(gpu)[off:]).cpu().numpy()
            want = np.zeros_like(got)
            assert lib.ia_row_slabs_host(np.ascontiguousarray(live).ctypes.data, len(live), want.ctypes.data) == 0
            for i, w in enumerate(expected_list(live)):
                if w is not None:
                    assert got[i] == w == want[i], (len(live), off, i)


def forward_case(gpu, operands, M, N, K, epilogue, qcols, must_filter, fp64=False):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    assert lib.ia_gemm_fwd_rows_filters(M, N, K) == (1 if must_filter else 0)
    x, w = operands["x"][:M, :K].contiguous(), operands["w"][:N, :K].contiguous()
    bias = operands["bias"][:N].contiguous() if epilogue != EPI_NONE else None
    scale = operands.get("col_scale", 0.18)
    kw = dict(epilogue=epilogue, bias=bias, scaled_cols=qcols, col_scale=scale if qcols else 1.0)
    sent = lambda: torch.full((M, N), SENTINEL, device=gpu, dtype=torch.bfloat16)
    dense = ops.gemm_fwd_slabs(x, w, None, **kw)          # row_live = NULL: the unfiltered call
    dense = dense if isinstance(dense, tuple) else (dense,)
    if fp64:
        found = []
        lin = x.double() @ w.double().t()
        if bias is not None:
            lin = lin + bias.double()[None]
            lin[:, :qcols] *= scale
        ref = torch.nn.functional.gelu(lin) if epilogue == EPI_BIAS_GELU else lin
        for name, live_np, live, rows in masks_on(gpu, M):
            if not rows.any():
                continue
            got = ops.gemm_fwd_slabs(x, w, live, **kw)
            got = got[0] if isinstance(got, tuple) else got
            err, err_dense = rel_err(got[rows], ref[rows]), rel_err(dense[0][rows], ref[rows])
            print(f"fwd epi {epilogue} {M}x{N}x{K} {name}: {int(rows.sum())} rows computed, vs fp64 {err:.3e} (unfiltered call, same rows: {err_dense:.3e})")
            assert err == err_dense, (M, N, K, name)
            found.append((("fwd", epilogue, M, N, K, name), err))
        return found
    for name, live_np, live, rows in masks_on(gpu, M):
        for fill in (True, False):
            got = ops.gemm_fwd_slabs(x, w, live, fill=fill, out=sent(), pre_out=sent() if epilogue == EPI_BIAS_GELU else None, **kw)
            got = got if isinstance(got, tuple) else (got,)
            tag = (M, N, K, name, fill)
            for g, d in zip(got, dense):
                assert torch.equal(g[rows], d[rows]), tag                       # rows of live slabs: the unfiltered call, bit for bit
                if must_filter and (~rows).any():
                    assert (g[~rows] == (0.0 if fill else SENTINEL)).all(), tag   # dead slabs: zeros, or not written
        # NaN in the input rows of dead slabs must not show
        if must_filter and (~rows).any():
            xp = torch.where(rows[:, None], x, torch.full_like(x, float("nan"))).contiguous()
            gp = ops.gemm_fwd_slabs(xp, w, live, fill=True, **kw)
            gp = gp if isinstance(gp, tuple) else (gp,)
            for g, d in zip(gp, dense):
                assert torch.equal(g[rows], d[rows]) and (g[~rows] == 0.0).all(), (M, N, K, name, "poisoned")


@pytest.mark.parametrize("epilogue", [EPI_NONE, EPI_BIAS_GELU], ids=["none", "bias_gelu"])
@pytest.mark.parametrize("M,N,K", BIG)
def test_fwd_slabs_equals_unfiltered(gpu, operands, M, N, K, epilogue):
    forward_case(gpu, operands, M, N, K, epilogue, 0, True)


@pytest.mark.parametrize("M,N,K", BIG_Q)
def test_fwd_slabs_scaled_columns(gpu, operands, M, N, K):
    forward_case(gpu, operands, M, N, K, EPI_BIAS, 1024, True)


@pytest.mark.parametrize("M,N,K", BIG_LA)
def test_fwd_slabs_lookahead_kernel(gpu, operands, M, N, K):
    forward_case(gpu, operands, M, N, K, EPI_NONE, 0, True)


@pytest.mark.parametrize("M", [264, 765, 1032])
def test_fwd_slabs_below_the_256_wide_kernel(gpu, operands, M):
    for _, N, K in [s for s in SMALL if s[0] == M]:
        forward_case(gpu, operands, M, N, K, EPI_NONE, 0, False)
        forward_case(gpu, operands, M, N, K, EPI_BIAS_GELU, 0, False)
        if N == 3072:
            forward_case(gpu, operands, M, N, K, EPI_BIAS, 1024, False)


def dgrad_case(gpu, operands, M, N, K, epilogue, w_kstrided, must_filter, fp64=False):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    assert lib.ia_gemm_dgrad_rows_filters(M, N, K) == (1 if must_filter else 0)
    wt = operands["w"][:N, :K].contiguous()                                    # [N_in, K_out]: the transposed shadow
    b = wt.t().contiguous() if w_kstrided else wt
    nan = lambda: torch.full((M, N), float("nan"), device=gpu, dtype=torch.bfloat16)
    sign = torch.where(torch.arange(K, device=gpu) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)
    found = []
    for name, live_np, live, rows in masks_on(gpu, M):
        keep = live[:, None].to(torch.bfloat16)
        dy = (operands["x"][:M, :K] * keep).contiguous()                       # the contract: dead rows of dY are zero ...
        aux = (operands["aux"][:M, :N] * keep).contiguous() if epilogue == EPI_ADD else None      # ... and of aux
        dense = ops.gemm(dy, b, b_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan())
        got = ops.gemm_dgrad_slabs(dy, b, live, w_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan())
        tag = (M, N, K, name)
        if fp64:
            if rows.any():
                ref = dy.double() @ wt.double().t()
                if aux is not None:
                    ref = ref + aux.double()
                err, err_dense = rel_err(got[rows], ref[rows]), rel_err(dense[rows], ref[rows])
                print(f"dgrad epi {epilogue} {M}x{N}x{K} {name}: vs fp64 {err:.3e} (unfiltered call, same rows: {err_dense:.3e})")
                assert err == err_dense, tag
                found.append((("dgrad", epilogue, w_kstrided) + tag, err))
            continue
        assert not torch.isnan(got).any(), tag                                 # every row was written
        assert torch.equal(got, dense), tag                                    # live slabs as computed, dead ones zero
        assert (got[~rows] == 0.0).all(), tag
        assert torch.equal(ops.gemm_dgrad_slabs(dy, b, None, w_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan()), dense), tag
        if must_filter and (~rows).any():                                      # large values in dead slabs are not read
            dyp = torch.where(rows[:, None], dy, sign[None, :]).contiguous()
            assert torch.equal(ops.gemm_dgrad_slabs(dyp, b, live, w_kstrided=w_kstrided, epilogue=epilogue, aux=aux, out=nan()), got), tag
    return found


@pytest.mark.parametrize("w_kstrided", [True, False], ids=["w_kstrided", "w_transposed"])
@pytest.mark.parametrize("epilogue", [EPI_NONE, EPI_ADD], ids=["none", "add"])
@pytest.mark.parametrize("M,N,K", BIG)
def test_dgrad_slabs_equals_unfiltered(gpu, operands, M, N, K, epilogue, w_kstrided):
    dgrad_case(gpu, operands, M, N, K, epilogue, w_kstrided, True)


@pytest.mark.parametrize("M,N,K", BIG_LA)
def test_dgrad_slabs_lookahead_kernel(gpu, operands, M, N, K):
    dgrad_case(gpu, operands, M, N, K, EPI_NONE, False, True)


@pytest.mark.parametrize("M", [264, 765, 1032])
def test_dgrad_slabs_below_the_256_wide_kernel(gpu, operands, M):
    for _, N, K in [s for s in SMALL if s[0] == M]:
        for epilogue in (EPI_NONE, EPI_ADD):
            dgrad_case(gpu, operands, M, N, K, epilogue, False, False)
            dgrad_case(gpu, operands, M, N, K, epilogue, True, False)


# ---- the live rows against fp64 (every instantiation, every BIG shape, every mask)
def fp64_errors(gpu, operands, with_gelu):
    gelu, linear = [], []
    for M, N, K in BIG:
        if with_gelu:
            gelu += forward_case(gpu, operands, M, N, K, EPI_BIAS_GELU, 0, True, fp64=True)
        linear += forward_case(gpu, operands, M, N, K, EPI_NONE, 0, True, fp64=True)
        for epilogue in (EPI_NONE, EPI_ADD):
            for w_kstrided in (False, True):
                linear += dgrad_case(gpu, operands, M, N, K, epilogue, w_kstrided, True, fp64=True)
    for M, N, K in BIG_Q:
        linear += forward_case(gpu, operands, M, N, K, EPI_BIAS, 1024, True, fp64=True)
    for M, N, K in BIG_LA:
        linear += forward_case(gpu, operands, M, N, K, EPI_NONE, 0, True, fp64=True)
        linear += dgrad_case(gpu, operands, M, N, K, EPI_NONE, False, True, fp64=True)
    return gelu, linear


def test_live_rows_against_fp64(gpu, operands):
    """The error of the rows of live slabs against fp64, as a fraction of the largest reference element, bound 2e-3
    (tests/test_gemm_wgrad_blocks_gpu.py), on the `exact` operands: there every output is a number bf16 holds, so the figure is the
    kernels' arithmetic and not the rounding of the store.  The store alone takes up to 2^-8 = 3.9e-3 of a value -- bf16 has an 8-bit
    significand; the bound comes from a test of fp32 outputs -- and normal operands measure just that, filtered call and unfiltered call
    alike: 1.9e-3 to 3.5e-3 on MI355X with every row live (3.09e-3 at 5100 x 2048 x 64, 3.46e-3 at K = 192, 2.37e-3 at K = 1024,
    2.19e-3 at 4096 x 128 in the look-ahead kernel, 1.92e-3 at 5120 x 3072 x 192 with scaled columns); on the exact operands: 0.  Those runs stay, held to what tests/test_kernels_gpu.py holds bf16 outputs to (2e-2, the GELU form against the
    exact function included).  Every figure of both runs is asserted equal to the unfiltered call's on the same rows."""
    _, linear = fp64_errors(gpu, operands["exact"], False)
    print("exact operands, linear forms: largest %.3e over %d cases" % (max(e for _, e in linear), len(linear)))
    assert all(e < 2e-3 for _, e in linear), max(linear, key=lambda t: t[1])
    gelu, normal = fp64_errors(gpu, operands, True)
    print("normal operands: GELU form %.3e, linear forms %.3e" % (max(e for _, e in gelu), max(e for _, e in normal)))
    assert all(e < 2e-2 for _, e in gelu + normal), max(gelu + normal, key=lambda t: t[1])


def test_pairs_without_a_kernel_form_are_refused(gpu):
    """The (filter kind, epilogue) pairs that have no kernel form return IA_ERR_UNSUPPORTED (-4) before anything is launched: the output
    keeps its sentinel.  M = 40, N = K = 128: the check precedes every launch, so the shape only has to pass argument validation."""
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import stream_ptr
    lib = _lib.load()
    M, N, K = 40, 128, 128
    EPI_BIAS_GELU_ACT, EPI_DGELU_COLSUM, UNSUPPORTED = 7, 6, -4
    x = torch.ones((M, K), device=gpu, dtype=torch.bfloat16)
    w = torch.ones((N, K), device=gpu, dtype=torch.bfloat16)
    aux = torch.ones((M, N), device=gpu, dtype=torch.bfloat16)
    bias = torch.ones(N, device=gpu)
    live = torch.ones(M, device=gpu, dtype=torch.uint8)
    out = torch.full((M, N), SENTINEL, device=gpu, dtype=torch.bfloat16)
    ws_bytes = max(lib.ia_gemm_slabs_workspace_bytes(M), lib.ia_gemm_fwd_rows_workspace_bytes(M), lib.ia_gemm_dgrad_rows_workspace_bytes(M, N, K))
    ws = torch.zeros(ws_bytes, device=gpu, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    for row_live in (p(live), None):
        assert lib.ia_gemm_fwd_slabs(p(x), K, p(w), K, p(out), N, M, N, K, EPI_BIAS_GELU_ACT, p(bias), None, 0, 1.0, row_live, 1, p(ws), ws_bytes,
                                     stream_ptr()) == UNSUPPORTED
        assert lib.ia_gemm_dgrad_slabs(p(x), K, p(w), 0, K, p(out), N, M, N, K, EPI_DGELU_COLSUM, p(aux), N, row_live, p(ws), ws_bytes,
                                       stream_ptr()) == UNSUPPORTED
        assert lib.ia_gemm_fwd_rows(p(x), K, p(w), K, p(out), N, M, N, K, EPI_ADD, p(bias), None, 0, 1.0, row_live, 1, p(ws), ws_bytes,
                                    stream_ptr()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and not bool(ws.any())
