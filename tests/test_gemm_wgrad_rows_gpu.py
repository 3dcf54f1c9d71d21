"""ia_gemm_wgrad_rows: the weight gradient dW = dY^T X that skips the 64-row k-tiles whose rows are all masked out, against the dense
call (ia_gemm_bf16, weight-gradient form) bit for bit, against fp64, and -- without timing anything -- for proof that the dead k-tiles
really are not read.

The filter lives in the 256 x 256-tile kernel; outputs too small for it take the 128-wide kernel and read every row
(ia_gemm_wgrad_rows_filters says which).  Both kinds are here: 256x256, 512x256 and 768x1024 with 1275 and 4080 rows run dense on either
side of the comparison (the plan of make_plan needs tiles x slabs >= 160 for the 256-wide kernel), so equality, the fp64 bound and the
NULL form are checked on them but a poisoned dead k-tile would rightly show; the three larger shapes are the smallest that reach the
256-wide kernel with k-slabs (1280x1024 x 4080 rows: 8 slabs of 8 k-tiles; 2560x2048 x 1275 rows: 2 slabs of 10, with a K tail) and
without (4352x4096 x 765 rows: one slab of 12 with a K tail, 272 tiles on 256 workgroups, so some walk the list twice).

fp64 bound: 2e-3 of the largest reference element, the bound tests/test_kernels_gpu.py holds fp32-output weight gradients to
(test_gemm_tn_wgrad)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BK = 64
SMALL = [(256, 256), (512, 256), (768, 1024)]
SHAPES = [(n_out, n_in, rows) for (n_out, n_in) in SMALL for rows in (1275, 4080)] + [(1280, 1024, 4080), (2560, 2048, 1275), (4352, 4096, 765)]
FILTERED = {(1280, 1024, 4080), (2560, 2048, 1275), (4352, 4096, 765)}


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def slab_tiles(n_out, n_in, rows):
    """k-tiles per k-slab of the plan both entry points use"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    nk = (rows + BK - 1) // BK
    splits = max(1, lib.ia_gemm_workspace_bytes(n_out, n_in, rows, 1) // (n_out * (n_in + 1) * 4))
    return nk, (nk + splits - 1) // splits


def patterns(n_out, n_in, rows):
    """name -> row_live (numpy uint8 [rows])"""
    nk, per = slab_tiles(n_out, n_in, rows)
    tile = lambda t: slice(t * BK, min(rows, (t + 1) * BK))
    out = {"all_live": np.ones(rows, np.uint8), "all_dead": np.zeros(rows, np.uint8)}
    # right-padded sequences of 255 positions, lengths 3 + U[8,48] + U[16,203] as the benchmark's synthetic data draws them
    rs = np.random.RandomState(2345)
    L = 255
    live = np.zeros((rows + L - 1) // L * L, np.uint8)
    for b in range(len(live) // L):
        live[b * L: b * L + 3 + rs.randint(8, 49) + rs.randint(16, 204)] = 1
    out["padded"] = live[:rows].copy()
    s = np.ones(rows, np.uint8)          # one slab dead (the second if there is one), its neighbours live
    first = per if nk > per else 0
    s[first * BK: min(rows, (first + per) * BK)] = 0
    out["slab_dead"] = s
    e = np.ones(rows, np.uint8)          # first and last k-tile of every slab dead
    for t0 in range(0, nk, per):
        e[tile(t0)] = 0
        e[tile(min(nk, t0 + per) - 1)] = 0
    out["slab_edges_dead"] = e
    t = np.ones(rows, np.uint8); t[tile(nk - 1)] = 0
    out["tail_dead"] = t
    t = np.zeros(rows, np.uint8); t[tile(nk - 1)] = 1; t[tile(0)] = 1
    out["tail_live"] = t
    o = np.zeros(rows, np.uint8); o[rows // 2 + 7] = 1
    out["one_row"] = o
    return out


@pytest.fixture(scope="module")
def operands(gpu):
    cache = {}

    def get(n_out, n_in, rows):
        key = (n_out, n_in, rows)
        if key not in cache:
            g = torch.Generator(device="cpu").manual_seed(rows + n_out)
            dy = torch.randn((rows, n_out), generator=g).to(gpu).to(torch.bfloat16)
            x = torch.randn((rows, n_in), generator=g).to(gpu).to(torch.bfloat16)
            cache.clear()            # one shape's operands at a time
            cache[key] = (dy, x)
        return cache[key]
    return get


@pytest.mark.parametrize("n_out,n_in,rows", SHAPES)
def test_wgrad_rows_matches_dense_and_skips_dead_ktiles(gpu, operands, n_out, n_in, rows):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    filtered = bool(lib.ia_gemm_wgrad_rows_filters(n_out, n_in, rows))
    assert filtered == ((n_out, n_in, rows) in FILTERED)       # the shapes meant to reach the filtering kernel do
    dy0, x = operands(n_out, n_in, rows)
    base = torch.full((n_out, n_in), 0.5, device=gpu, dtype=torch.float32)
    for name, live_np in patterns(n_out, n_in, rows).items():
        live = torch.from_numpy(live_np).to(gpu)
        dy = (dy0 * live[:, None].to(dy0.dtype)).contiguous()          # the contract: dead rows of dY are zero
        dense = ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True)
        got = ops.gemm_wgrad_rows(dy, x, live)
        ref = dy.double().t() @ x.double()
        err = rel_err(got, ref)
        nk = (rows + BK - 1) // BK
        dead_tile = np.array([not live_np[t * BK: (t + 1) * BK].any() for t in range(nk)])
        print(f"{n_out}x{n_in} rows {rows} {name}: {nk - int(dead_tile.sum())} of {nk} k-tiles live, vs fp64 {err:.2e} (dense {rel_err(dense, ref):.2e})")
        assert torch.equal(got, dense), name                            # 1. the dense path, bit for bit (+-0 compare equal)
        if live_np.any():
            assert err < 2e-3, (name, err)                              # 2. fp64, the bound of test_gemm_tn_wgrad
        else:
            assert got.abs().max().item() == 0.0, name                  # all dead: exactly zero ...
        acc = ops.gemm_wgrad_rows(dy, x, live, out=base.clone(), accumulate=True)
        assert torch.equal(acc, ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True, out=base.clone(), accumulate=True)), name
        if not live_np.any():
            assert torch.equal(acc, base), name                         # ... and an accumulating call leaves C as it was
        assert torch.equal(ops.gemm_wgrad_rows(dy, x, None), dense), name   # 4. NULL = the dense call
        if filtered:
            # 3. large finite values in the rows of k-tiles that are dead as a whole (rows of partly live k-tiles stay zero: the contract
            # needs them zero): a kernel that read those k-tiles could not return the clean result
            poison_rows = torch.from_numpy(np.repeat(dead_tile, BK)[:rows]).to(gpu)
            if dead_tile.any():
                sign = torch.where(torch.arange(n_out, device=gpu) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)
                dyp = torch.where(poison_rows[:, None], sign[None, :], dy).contiguous()
                assert torch.equal(ops.gemm_wgrad_rows(dyp, x, live), got), name
                assert not torch.equal(ops.gemm(dyp, x, a_kstrided=True, b_kstrided=True, out_f32=True), got), name    # (the poison is seen by a dense read)


@pytest.mark.parametrize("rows", [1275, 4080, 2048 * 64 + 100])
def test_ktile_mask_kernel_matches_numpy(gpu, rows):
    from item_alignment_amd import ops
    rs = np.random.RandomState(rows)
    live = (rs.rand(rows) < 0.01).astype(np.uint8)
    live[5 * BK: 9 * BK] = 0
    live[-1] = 1
    for off in (0, 3):                     # an unaligned row_live pointer too
        buf = torch.zeros(rows + off, dtype=torch.uint8)
        buf[off:] = torch.from_numpy(live)
        got = ops.ktile_mask(buf.to(gpu)[off:]).cpu().numpy().view(np.uint32)
        nk = (rows + BK - 1) // BK
        bits = np.array([live[t * BK: (t + 1) * BK].any() for t in range(nk)] + [False] * (-nk % 32))
        want = (bits.reshape(-1, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(1).astype(np.uint32)
        assert np.array_equal(got, want)
