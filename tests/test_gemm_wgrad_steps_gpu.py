"""ia_gemm_wgrad_steps: the weight gradient dW = dY^T X over the live 16-row steps of k (four to a k-tile of the 256-wide kernel's loop),
bit for bit against the dense call and against ia_gemm_wgrad_blocks, with NaN in X wherever a whole step is dead -- a kernel that read
one such row could not return the dense result.

Shapes: the smallest the 256-wide split-K plan takes (tiles x splits >= 160 with splits <= k-tiles / 8), every M_rows with a partial last
step (not a multiple of 16, so not of 64 either): 1024x512 x 10267 rows, the text-like 1024x1024 x 5389 and 768x1280 x 5705.  All three
walk steps (ia_gemm_wgrad_walk == 2).  4096x4096 x 32845 rows is the other side of step_mask_fits: 256 tiles leave the plan one k-slab
of 514 k-tiles, two more than a lane's mask words cover, so the call takes the block walk from the block mask of its step mask."""
import numpy as np
import pytest
import torch

from wgrad_masks import patterns as ktile_patterns, slab_tiles

pytestmark = pytest.mark.gpu

BK, STEP = 64, 16
SHAPES = [(1024, 512, 10267), (1024, 1024, 5389), (768, 1280, 5705)]
FAR_SHAPE = (4096, 4096, 32845)


def numpy_steps(live_np, rows_per_bit=STEP):
    """the mask words from a numpy OR over each run of rows_per_bit rows"""
    n = (len(live_np) + rows_per_bit - 1) // rows_per_bit
    bits = np.zeros((n + 31) // 32 * 32, np.uint8)
    padded = np.zeros(n * rows_per_bit, np.uint8)
    padded[:len(live_np)] = live_np
    bits[:n] = padded.reshape(n, rows_per_bit).any(axis=1)
    return (bits.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def patterns(n_out, n_in, rows):
    """name -> row_live (numpy uint8 [rows]): the k-tile patterns of tests/wgrad_masks.py and the ones only a walk by fours of 16-row steps can get wrong"""
    out = dict(ktile_patterns(n_out, n_in, rows))
    nk, per = slab_tiles(n_out, n_in, rows)
    ns, n_slabs = (rows + STEP - 1) // STEP, (nk + per - 1) // per
    assert rows % STEP != 0 and n_slabs >= 3
    steps = lambda keep: np.repeat(np.array([1 if keep(s) else 0 for s in range(ns)], np.uint8), STEP)[:rows].copy()
    first_of = lambda sl: 4 * sl * per
    count_of = lambda sl: min(ns, 4 * (sl + 1) * per) - first_of(sl)
    slab_of = lambda s: (s // 4) // per
    # every second step: each trip gathers its four steps from four different k-tiles
    out["every_second_step"] = steps(lambda s: s % 2 == 1)
    # live counts of 1, 2 and 3 mod 4, slab after slab: all live, less the steps behind the slab's first that bring the count there
    def drop(s):
        sl = slab_of(s)
        return 0 < s - first_of(sl) <= (count_of(sl) - (sl % 3 + 1)) % 4
    out["counts_1_2_3_mod_4"] = steps(lambda s: not drop(s))
    for sl in range(n_slabs):
        n = sum(out["counts_1_2_3_mod_4"][s * STEP: (s + 1) * STEP].any() for s in range(first_of(sl), first_of(sl) + count_of(sl)))
        assert n % 4 == sl % 3 + 1, (sl, n)
    # one live step in every slab but the second, which has none between two that have
    out["one_step_per_slab_one_empty"] = steps(lambda s: slab_of(s) != 1 and s == first_of(slab_of(s)) + min(5, count_of(slab_of(s)) - 1))
    # live runs of 58 rows across every slab boundary, 37 rows in front of it and 21 behind: partly live steps at both ends
    r = np.zeros(rows, np.uint8)
    for sl in range(1, n_slabs):
        r[sl * per * BK - 37: sl * per * BK + 21] = 1
    out["runs_over_slab_boundaries"] = r
    out["partial_last_step_only"] = steps(lambda s: s == ns - 1)
    return out


def poisoned(x, live_np, gpu):
    """x with NaN in every row of a step without a live row; the dead rows of partly live steps keep their finite values"""
    rows = len(live_np)
    ns = (rows + STEP - 1) // STEP
    dead_step = np.array([not live_np[s * STEP: (s + 1) * STEP].any() for s in range(ns)])
    mark = torch.from_numpy(np.repeat(dead_step, STEP)[:rows]).to(gpu)
    return torch.where(mark[:, None], torch.full_like(x, float("nan")), x).contiguous(), int(ns - dead_step.sum()), ns


def check(gpu, dy0, x, name, live_np, walk):
    from item_alignment_amd import ops
    n_out, n_in = dy0.shape[1], x.shape[1]
    live = torch.from_numpy(live_np).to(gpu)
    smask, bmask = ops.kstep_mask(live), ops.kblock_mask(live)
    assert np.array_equal(smask.cpu().numpy().view(np.uint32), numpy_steps(live_np)), name
    dy = (dy0 * live[:, None].to(dy0.dtype)).contiguous()              # the contract: dead rows of dY are zero
    xp, n_live, ns = poisoned(x, live_np, gpu)
    base = torch.full((n_out, n_in), 0.5, device=gpu, dtype=torch.float32)
    dense = ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True)
    dense_acc = ops.gemm(dy, x, a_kstrided=True, b_kstrided=True, out_f32=True, out=base.clone(), accumulate=True)
    print(f"{n_out}x{n_in} rows {len(live_np)} {name}: {n_live} of {ns} steps live")
    # the block walk reads the dead steps of its partly live blocks: it gets the clean x
    got = ops.gemm_wgrad_steps(dy, xp if walk == 2 else x, smask)
    assert torch.isfinite(got).all(), name
    assert torch.equal(got, dense), name
    assert torch.equal(got, ops.gemm_wgrad_blocks(dy, x, bmask)), name
    acc = ops.gemm_wgrad_steps(dy, xp if walk == 2 else x, smask, out=base.clone(), accumulate=True)
    assert torch.equal(acc, dense_acc), name
    assert torch.equal(acc, ops.gemm_wgrad_blocks(dy, x, bmask, out=base.clone(), accumulate=True)), name
    if not live_np.any():
        assert got.abs().max().item() == 0.0 and torch.equal(acc, base), name
    assert torch.equal(ops.gemm_wgrad_steps(dy, x, None), dense), name      # NULL = the dense call


@pytest.mark.parametrize("n_out,n_in,rows", SHAPES)
def test_wgrad_steps_matches_dense_and_blocks(gpu, n_out, n_in, rows):
    from item_alignment_amd import _lib
    lib = _lib.load()
    assert lib.ia_gemm_wgrad_walk(n_out, n_in, rows) == 2               # the step walk
    g = torch.Generator(device="cpu").manual_seed(rows + n_out)
    dy0 = torch.randn((rows, n_out), generator=g).to(gpu).to(torch.bfloat16)
    x = torch.randn((rows, n_in), generator=g).to(gpu).to(torch.bfloat16)
    for name, live_np in patterns(n_out, n_in, rows).items():
        check(gpu, dy0, x, name, live_np, 2)


def test_wgrad_steps_slab_too_long_takes_the_block_walk(gpu):
    from item_alignment_amd import _lib
    lib = _lib.load()
    n_out, n_in, rows = FAR_SHAPE
    nk, per = slab_tiles(n_out, n_in, rows)
    assert per == nk == 514 and lib.ia_gemm_wgrad_walk(n_out, n_in, rows) == 1 and lib.ia_gemm_wgrad_rows_filters(n_out, n_in, rows) == 1
    g = torch.Generator(device=gpu).manual_seed(7)
    dy0 = torch.randn((rows, n_out), generator=g, device=gpu, dtype=torch.bfloat16)
    x = torch.randn((rows, n_in), generator=g, device=gpu, dtype=torch.bfloat16)
    pats = ktile_patterns(n_out, n_in, rows)
    every_second = np.repeat((np.arange((rows + STEP - 1) // STEP) % 2).astype(np.uint8), STEP)[:rows].copy()
    for name, live_np in (("padded", pats["padded"]), ("every_second_step", every_second)):
        check(gpu, dy0, x, name, live_np, 1)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 16 * 77 + 1, 5389, 130560, 2048 * 64 + 100])
def test_kstep_mask_kernel_matches_host_and_numpy(gpu, rows):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    rs = np.random.RandomState(rows)
    live = (rs.rand(rows) < 0.03).astype(np.uint8)
    live[5 * STEP: 9 * STEP] = 0
    live[-1] = 1
    want = numpy_steps(live)
    host = np.full(lib.ia_kstep_mask_bytes(rows) // 4, 0x5A5A5A5A, np.uint32)
    assert lib.ia_kstep_mask_host(live.ctypes.data, rows, host.ctypes.data) == 0
    assert np.array_equal(host, want)
    for off in (0, 3):                     # an unaligned row_live pointer too
        buf = torch.zeros(rows + off, dtype=torch.uint8)
        buf[off:] = torch.from_numpy(live)
        got = ops.kstep_mask(buf.to(gpu)[off:]).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want)
