"""ia_gemm_wgrad_rows: the weight gradient dW = dY^T X that skips the 32-row blocks of k whose rows are all masked out (the entry builds the
block mask from the rows' live bytes, then walks it as ia_gemm_wgrad_blocks does), against the dense call (ia_gemm_bf16, weight-gradient
form) bit for bit, against fp64, and -- without timing anything -- for proof that the dead blocks really are not read.

The filter lives in the 256 x 256-tile kernel; outputs too small for it take the 128-wide kernel and read every row
(ia_gemm_wgrad_rows_filters says which).  Both kinds are here: 256x256, 512x256 and 768x1024 with 1275 and 4080 rows run dense on either
side of the comparison (the plan of make_plan needs tiles x slabs >= 160 for the 256-wide kernel), so equality, the fp64 bound and the
NULL form are checked on them but a poisoned dead block would rightly show; the three larger shapes are the smallest that reach the
256-wide kernel with k-slabs (1280x1024 x 4080 rows: 8 slabs of 8 k-tiles; 2560x2048 x 1275 rows: 2 slabs of 10, with a K tail) and
without (4352x4096 x 765 rows: one slab of 12 with a K tail, 272 tiles on 256 workgroups, so some walk the list twice).

fp64 bound: 2e-3 of the largest reference element, the bound tests/test_kernels_gpu.py holds fp32-output weight gradients to
(test_gemm_tn_wgrad)."""
import numpy as np
import pytest
import torch

from wgrad_masks import patterns, rel_err

pytestmark = pytest.mark.gpu

BLK = 32
SMALL = [(256, 256), (512, 256), (768, 1024)]
SHAPES = [(n_out, n_in, rows) for (n_out, n_in) in SMALL for rows in (1275, 4080)] + [(1280, 1024, 4080), (2560, 2048, 1275), (4352, 4096, 765)]
FILTERED = {(1280, 1024, 4080), (2560, 2048, 1275), (4352, 4096, 765)}


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
        nb = (rows + BLK - 1) // BLK
        dead_blk = np.array([not live_np[b * BLK: (b + 1) * BLK].any() for b in range(nb)])
        print(f"{n_out}x{n_in} rows {rows} {name}: {nb - int(dead_blk.sum())} of {nb} blocks live, vs fp64 {err:.2e} (dense {rel_err(dense, ref):.2e})")
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
            # 3. +-1e4 in dY and NaN in X in the rows of every dead 32-row block, the dead halves of partly live k-tiles included (dead
            # rows of a partly live block stay zero: the contract needs them zero): a kernel that read one of those blocks could not
            # return the clean result
            poison_rows = torch.from_numpy(np.repeat(dead_blk, BLK)[:rows]).to(gpu)
            if dead_blk.any():
                sign = torch.where(torch.arange(n_out, device=gpu) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)
                dyp = torch.where(poison_rows[:, None], sign[None, :], dy).contiguous()
                xp = torch.where(poison_rows[:, None], torch.full_like(x, float("nan")), x).contiguous()
                assert torch.equal(ops.gemm_wgrad_rows(dyp, xp, live), got), name
                dense_p = ops.gemm(dyp, xp, a_kstrided=True, b_kstrided=True, out_f32=True)
                assert not torch.equal(dense_p, got) and not torch.isfinite(dense_p).all(), name    # (the poison is seen by a dense read)
