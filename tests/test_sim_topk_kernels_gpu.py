"""The similarity top-k kernels (ia_sim_rows_bf16, ia_sim_topk; csrc/simtopk.hip) against tests/simtopk_reference.py.

On exact operands (whole numbers in [-4, 4], D <= 1024: every partial sum is a whole number below 2^24, so the fp32 accumulation is exact
in any order) ids and scores are compared bit for bit with the fp64 selection, at the edges of the 128-candidate tile, of the 64-element
k stage, of the 128 / 256-query tile and of both kernel forms (k <= 32 and above), for every split count, with and without skipped
candidates.  On random bf16 operands the result has to pass check_topk with the derived accumulator bar and to be the same bits for
every split count and on a repeated call."""
import numpy as np
import pytest
import torch

import fp64_bars
import simtopk_reference as SR

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SPLITS = (1, 2, 7, 0)


def _R():
    from item_alignment_amd import retrieval
    return retrieval


def _prepared(x, dev):
    """bf16 [n, pitch] rows of the (bf16-exact) fp32 matrix x, built with torch alone"""
    R = _R()
    out = torch.zeros(x.shape[0], R.row_pitch(x.shape[1]), dtype=BF16)
    out[:, :x.shape[1]] = x.to(BF16)
    return out.to(dev)


def _ints(seed, n, D):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (n, D), generator=g).to(F32)


def _skips(B, n):
    b = np.arange(B)
    return np.where(b % 5 == 4, -1, (b * 7) % n).astype(np.int64)


def _bits_equal(idx, score, want_idx, want_score, what):
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(idx, want_idx), (what, "ids", np.argwhere(idx != want_idx)[:4])
    assert np.array_equal(score.view(np.int32), want_score.view(np.int32)), (what, "scores", np.argwhere(score != want_score)[:4])


# ------------------------------------------------------------------------------------------------ exact operands
@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("D", [8, 64, 72, 200, 768])
def test_exact_operands_bit_equal(gpu, D, B):
    R = _R()
    q, c = _ints(10 + D, B, D), _ints(20 + D, 1000, D)
    s64 = SR.scores_fp64(q, c)
    assert np.abs(s64).max() < 2 ** 24
    qd, cd = _prepared(q, gpu), _prepared(c, gpu)
    for n in (1, 5, 127, 128, 129, 257, 1000):
        cn = cd[:n].contiguous()
        for skip in (None, _skips(B, n)):                      # n = 1: the only candidate of query 0 is skipped
            for k in (1, 10, 64):                              # k > n included
                want = SR.select(s64[:, :n].astype(np.float32), k, skip)
                for ms in SPLITS:
                    got = R.sim_topk(qd, cn, D, k, skip=skip, max_splits=ms)
                    _bits_equal(*got, *want, (D, B, n, k, ms, skip is not None))
    only = R.sim_topk(qd[:1], cd[:1].contiguous(), D, 10, skip=np.array([0]))
    assert (only[0] == -1).all() and torch.isneginf(only[1]).all()


@pytest.mark.parametrize("k", [10, 64])
def test_many_tiles(gpu, k):
    """300 000 candidates, 2 344 tiles: several tiles per split in every split, the rows full of ties"""
    R = _R()
    q, c = _ints(1, 3, 8), _ints(2, 300000, 8)
    skip = np.array([-1, 299999, 4])
    want = SR.select(SR.scores_fp64(q, c).astype(np.float32), k, skip)
    qd, cd = _prepared(q, gpu), _prepared(c, gpu)
    for ms in (0, 3):
        _bits_equal(*R.sim_topk(qd, cd, 8, k, skip=skip, max_splits=ms), *want, (k, ms))


@pytest.mark.parametrize("k", [10, 64])
def test_duplicate_rows_come_out_lowest_id_first(gpu, k):
    R = _R()
    g = torch.Generator().manual_seed(5)
    distinct = torch.nn.functional.normalize(torch.randn(40, 72, generator=g), dim=1).to(BF16).to(F32)
    group = torch.randint(0, 40, (1000,), generator=g)
    c, q = distinct[group], torch.nn.functional.normalize(torch.randn(130, 72, generator=g), dim=1).to(BF16).to(F32)
    s64, bars = SR.scores_fp64(q, c), SR.bar(q, c, R.row_pitch(72))
    qd, cd = _prepared(q, gpu), _prepared(c, gpu)
    group = group.numpy()
    first = None
    for ms in SPLITS:
        idx, score = (t.cpu().numpy() for t in R.sim_topk(qd, cd, 72, k, max_splits=ms))
        SR.check_topk(idx, score, s64, bars, k)
        for b in range(130):
            got = set(idx[b].tolist())
            for a, cid in enumerate(idx[b]):
                same = np.nonzero(group == group[cid])[0]
                assert all(int(o) in got for o in same[same < cid]), ("a duplicate with a lower id is left out", ms, b, cid)
                if a and group[idx[b, a - 1]] == group[cid]:
                    assert score[b, a - 1].view(np.int32) == score[b, a].view(np.int32) and idx[b, a - 1] < cid
        if first is None:
            first = (idx, score)
        assert np.array_equal(first[0], idx) and np.array_equal(first[1].view(np.int32), score.view(np.int32)), ms


# ------------------------------------------------------------------------------------------------ random bf16 operands
@pytest.mark.parametrize("D", [72, 768])
def test_random_operands_within_the_bar_and_reproducible(gpu, D):
    R = _R()
    g = torch.Generator().manual_seed(D)
    q = torch.nn.functional.normalize(torch.randn(130, D, generator=g), dim=1).to(BF16).to(F32)
    c = torch.nn.functional.normalize(torch.randn(1000, D, generator=g), dim=1).to(BF16).to(F32)
    skip = _skips(130, 1000)
    s64, bars = SR.scores_fp64(q, c), SR.bar(q, c, R.row_pitch(D))
    qd, cd = _prepared(q, gpu), _prepared(c, gpu)
    for k in (10, 64):
        first = None
        for ms in SPLITS + (0,):                               # the last one: the same call twice
            idx, score = (t.cpu().numpy() for t in R.sim_topk(qd, cd, D, k, skip=skip, max_splits=ms))
            if first is None:
                SR.check_topk(idx, score, s64, bars, k, skip)
                first = (idx, score)
            assert np.array_equal(first[0], idx) and np.array_equal(first[1].view(np.int32), score.view(np.int32)), (k, ms)


# ------------------------------------------------------------------------------------------------ pitched buffers
def test_nothing_outside_the_buffers_is_read_or_written(gpu):
    from item_alignment_amd import _lib
    R = _R()
    lib = _lib.load()
    B, n, D, k, G = 130, 257, 72, 10, 4096
    pitch = R.row_pitch(D)
    q, c = _ints(1, B, D), _ints(2, n, D)
    want = SR.select(SR.scores_fp64(q, c).astype(np.float32), k, None)
    ops = torch.full((G + B * pitch + G + n * pitch + G,), float("nan"), device=gpu, dtype=BF16)
    qd = ops[G:G + B * pitch].view(B, pitch)
    cd = ops[2 * G + B * pitch:2 * G + (B + n) * pitch].view(n, pitch)
    qd.copy_(_prepared(q, gpu))
    cd.copy_(_prepared(c, gpu))
    idx_buf = torch.full((G + B * k + G,), -777, device=gpu, dtype=torch.int64)
    sc_buf = torch.full((G + B * k + G,), 12345.0, device=gpu, dtype=F32)
    nbytes = lib.ia_sim_topk_workspace_bytes(B, D, n, k, 0)
    ws = torch.full((G + nbytes + G,), 0x5A, device=gpu, dtype=torch.uint8)
    rc = lib.ia_sim_topk(qd.data_ptr(), cd.data_ptr(), B, D, n, None, k, 0, idx_buf[G:].data_ptr(), sc_buf[G:].data_ptr(), ws[G:].data_ptr(),
                         nbytes, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    _bits_equal(idx_buf[G:G + B * k].view(B, k), sc_buf[G:G + B * k].view(B, k), *want, "pitched")
    assert not torch.isnan(sc_buf).any()
    for buf, fill in ((idx_buf, -777), (sc_buf, 12345.0), (ws, 0x5A)):
        assert (buf[:G] == fill).all() and (buf[-G:] == fill).all()
    assert torch.isnan(ops[:G]).all() and torch.isnan(ops[G + B * pitch:2 * G + B * pitch]).all() and torch.isnan(ops[-G:]).all()


def test_empty_sides_and_argument_errors_leave_the_outputs_alone(gpu):
    from item_alignment_amd import _lib
    R = _R()
    lib = _lib.load()
    B, n, D, k = 5, 9, 8, 3
    qd, cd = _prepared(_ints(1, B, D), gpu), _prepared(_ints(2, n, D), gpu)
    idx = torch.full((B, k), -777, device=gpu, dtype=torch.int64)
    score = torch.full((B, k), 12345.0, device=gpu, dtype=F32)
    ws = torch.empty(1 << 16, device=gpu, dtype=torch.uint8)

    def call(q=qd.data_ptr(), c=cd.data_ptr(), B=B, D=D, n=n, k=k, ms=0, i=idx.data_ptr(), s=score.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        rc = lib.ia_sim_topk(q, c, B, D, n, None, k, ms, i, s, w, wb, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for bad in (dict(q=None), dict(c=None), dict(i=None), dict(s=None), dict(w=None), dict(k=0), dict(k=65), dict(D=0), dict(B=-1), dict(n=-1),
                dict(ms=-1), dict(wb=8), dict(c=cd.data_ptr() + 2)):
        assert call(**bad) == -1, bad
        assert (idx == -777).all() and (score == 12345.0).all(), bad
    assert call(B=0) == 0
    assert (idx == -777).all() and (score == 12345.0).all()
    assert call(n=0, w=None, wb=0) == 0                        # no candidates: every slot unused
    assert (idx == -1).all() and torch.isneginf(score).all()
    i2, s2 = R.sim_topk(qd, cd[:0], D, k)
    assert (i2 == -1).all() and torch.isneginf(s2).all() and i2.shape == (B, k)
    i3, s3 = R.sim_topk(qd[:0], cd, D, k)
    assert i3.shape == (0, k) and s3.shape == (0, k)
    with pytest.raises(ValueError):
        R.sim_topk(qd, cd, D, 65)
    with pytest.raises(ValueError):
        R.sim_topk(qd, cd, D + 64, k)


# ------------------------------------------------------------------------------------------------ ia_sim_rows_bf16
@pytest.mark.parametrize("D", [3, 64, 72, 3072])
def test_rows_kernel(gpu, D):
    R = _R()
    rows, ld = 9, D + 5
    g = torch.Generator().manual_seed(D)
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :D] = torch.randn(rows, D, generator=g) * 3.0
    buf[4, :D] = 0.0                                           # an all-zero row
    x = buf.to(gpu)[:, :D]                                     # ldx > D, NaN in the padding of x
    assert x.stride(0) == ld
    pitch = R.row_pitch(D)
    assert pitch >= D and pitch % 64 == 0
    for normalize in (0, 1):
        out = R.prepare_rows(x, normalize)
        assert out.shape == (rows, pitch) and out.dtype == BF16
        assert (out[:, D:].view(torch.int16) == 0).all(), "pad columns"
        want = SR.rows_fp64(buf[:, :D], normalize)
        if normalize:
            fp64_bars.bf16_close(f"rows D={D}", out[:, :D], want, a=0)
        else:
            fp64_bars.bits(f"rows D={D}", out[:, :D], want)
        assert (out[4].view(torch.int16) == 0).all(), "an all-zero row"
    one = R.prepare_rows(x[:1], 1)                             # a single row
    assert torch.equal(one, R.prepare_rows(x, 1)[:1])
