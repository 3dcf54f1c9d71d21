"""ia_gemm_wgrad_blocks: the weight gradient dW = dY^T X over the live 32-row blocks of k (two to a k-tile of the 256-wide kernel's loop),
against the dense call bit for bit, against fp64, and -- without timing anything -- for proof that dead blocks are not read, the dead
halves of partly live 64-row k-tiles included.

The three shapes are the smallest that reach the 256-wide kernel (tests/test_gemm_wgrad_rows_gpu.py): 1280x1024 x 4080 rows (8 k-slabs of 8
k-tiles; 4080 = 127 * 32 + 16), 2560x2048 x 1275 rows (2 slabs of 10 with a K tail; 1275 = 39 * 32 + 27) and 4352x4096 x 765 rows (one slab,
272 tiles on 256 workgroups; 765 = 23 * 32 + 29).  fp64 bound: 2e-3 of the largest reference element (test_gemm_tn_wgrad)."""
import numpy as np
import pytest
import torch

from wgrad_masks import patterns as ktile_patterns, rel_err, slab_tiles

pytestmark = pytest.mark.gpu

BK, BLK = 64, 32
SHAPES = [(1280, 1024, 4080), (2560, 2048, 1275), (4352, 4096, 765)]


def patterns(n_out, n_in, rows):
    """name -> row_live (numpy uint8 [rows]): the patterns laid out on 64-row k-tiles (tests/wgrad_masks.py) and the ones only a 32-row walk can get wrong"""
    out = dict(ktile_patterns(n_out, n_in, rows))
    nk, per = slab_tiles(n_out, n_in, rows)
    nb = (rows + BLK - 1) // BLK
    assert rows % BLK != 0                              # every shape has a partial last block
    blocks = lambda keep: np.repeat(np.array([1 if keep(b) else 0 for b in range(nb)], np.uint8), BLK)[:rows].copy()
    out["lower_halves"] = blocks(lambda b: b % 2 == 0)
    out["upper_halves"] = blocks(lambda b: b % 2 == 1)
    out["alternating_halves"] = blocks(lambda b: b % 2 == (b // 2) % 2)
    slab_of = lambda b: (b // 2) // per
    first_of = lambda s: 2 * s * per
    count_of = lambda s: min(nb, 2 * (s + 1) * per) - first_of(s)
    # all live, less the second block of every slab that holds an even number of blocks
    out["odd_count_per_slab"] = blocks(lambda b: not (count_of(slab_of(b)) % 2 == 0 and b == first_of(slab_of(b)) + 1))
    out["one_block_per_slab"] = blocks(lambda b: b == min(first_of(slab_of(b)) + 3, first_of(slab_of(b)) + count_of(slab_of(b)) - 1))
    out["partial_last_block_only"] = blocks(lambda b: b == nb - 1)
    out["partial_last_block_dead"] = blocks(lambda b: b != nb - 1)
    for s in range((nk + per - 1) // per):
        n_odd = sum(out["odd_count_per_slab"][b * BLK: (b + 1) * BLK].any() for b in range(first_of(s), first_of(s) + count_of(s)))
        n_one = sum(out["one_block_per_slab"][b * BLK: (b + 1) * BLK].any() for b in range(first_of(s), first_of(s) + count_of(s)))
        assert n_odd % 2 == 1 and n_one == 1, (s, n_odd, n_one)
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


def host_mask(live_np):
    from item_alignment_amd import _lib
    lib = _lib.load()
    m = np.full(lib.ia_kblock_mask_bytes(len(live_np)) // 4, 0x5A5A5A5A, np.uint32)
    assert lib.ia_kblock_mask_host(np.ascontiguousarray(live_np).ctypes.data, len(live_np), m.ctypes.data) == 0
    return m


@pytest.mark.parametrize("n_out,n_in,rows", SHAPES)
def test_wgrad_blocks_matches_dense_and_skips_dead_blocks(gpu, operands, n_out, n_in, rows):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    assert lib.ia_gemm_wgrad_rows_filters(n_out, n_in, rows) == 1       # the 256-wide kernel, whose k loop the walk lives in
    dy0, x = operands(n_out, n_in, rows)
    base = torch.full((n_out, n_in), 0.5, device=gpu, dtype=torch.float32)
    nb = (rows + BLK - 1) // BLK
    sign = torch.where(torch.arange(n_out, device=gpu) % 2 == 0, 1e4, -1e4).to(torch.bfloat16)
    for name, live_np in patterns(n_out, n_in, rows).items():
        live = torch.from_numpy(live_np).to(gpu)
        # the block-mask kernel against the host twin
        mask = ops.kblock_mask(live)
        assert np.array_equal(mask.cpu().numpy().view(np.uint32), host_mask(live_np)), name
        dy = (dy0 * live[:, None].to(dy0.dtype)).contiguous()          # the contract: dead rows of dY are zero
        dense = ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True)
        got = ops.gemm_wgrad_blocks(dy, x, mask)
        ref = dy.double().t() @ x.double()
        err = rel_err(got, ref)
        dead_blk = np.array([not live_np[b * BLK: (b + 1) * BLK].any() for b in range(nb)])
        print(f"{n_out}x{n_in} rows {rows} {name}: {nb - int(dead_blk.sum())} of {nb} blocks live, vs fp64 {err:.2e} (dense {rel_err(dense, ref):.2e})")
        assert torch.equal(got, dense), name                            # 1. the dense path, bit for bit
        if live_np.any():
            assert err < 2e-3, (name, err)                              # 2. fp64, the bound of test_gemm_tn_wgrad
        else:
            assert got.abs().max().item() == 0.0, name                  # all dead: exactly zero ...
        acc = ops.gemm_wgrad_blocks(dy, x, mask, out=base.clone(), accumulate=True)
        assert torch.equal(acc, ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True, out=base.clone(), accumulate=True)), name
        if not live_np.any():
            assert torch.equal(acc, base), name                         # ... and an accumulating call leaves C as it was
        assert torch.equal(ops.gemm_wgrad_blocks(dy, x, None), dense), name   # NULL = the dense call
        # 3. the skip: NaN in X and +-1e4 in dY in the rows of every dead 32-row block, the dead halves of partly live k-tiles included.
        # A kernel that read one of them could not return the clean result; the dense kernel reads them all.
        if dead_blk.any():
            poison = torch.from_numpy(np.repeat(dead_blk, BLK)[:rows]).to(gpu)
            dyp = torch.where(poison[:, None], sign[None, :], dy).contiguous()
            xp = torch.where(poison[:, None], torch.full_like(x, float("nan")), x).contiguous()
            assert torch.equal(ops.gemm_wgrad_blocks(dyp, xp, mask), got), name
            assert torch.equal(ops.gemm_wgrad_blocks(dyp, xp, mask, out=base.clone(), accumulate=True), acc), name
            assert not torch.isfinite(ops.gemm(dyp, xp, a_kstrided=True, b_kstrided=True, out_f32=True)).all(), name


@pytest.mark.parametrize("rows", [1, 31, 33, 1275, 4080, 130560, 2048 * 64 + 100])
def test_kblock_mask_kernel_matches_host(gpu, rows):
    from item_alignment_amd import ops
    rs = np.random.RandomState(rows)
    live = (rs.rand(rows) < 0.02).astype(np.uint8)
    live[5 * BLK: 9 * BLK] = 0
    live[-1] = 1
    for off in (0, 3):                     # an unaligned row_live pointer too
        buf = torch.zeros(rows + off, dtype=torch.uint8)
        buf[off:] = torch.from_numpy(live)
        got = ops.kblock_mask(buf.to(gpu)[off:]).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, host_mask(live))
