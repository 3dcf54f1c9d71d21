"""ia_gemm_fwd_rows: the forward GEMM Y = X W^T (+ epilogue) that computes only the 32-row blocks holding a live row, against the
unfiltered call (ia_gemm_bf16 / ia_gemm_bf16_qscale) on the same inputs, element for element.

Shapes: the geometry and the seven masks of tests/test_gemm_dgrad_rows_gpu.py -- M = 20 x 255 = 5100 rows (159 whole blocks and one of
12 rows; 5100 is no multiple of 128, so the last rows take the dense kernel's guarded epilogue), N = 2048: 160 tiles of 256 x 256, the
smallest plan the 256-wide kernel takes (ia_gemm_fwd_rows_filters is asserted); K = 64 (one k-tile), 192 (three) and 1024.  Epilogues:
BIAS without scaled columns, BIAS with 1024 of N = 3072 columns scaled (the QKV projection's form), BIAS_GELU with its second output,
BIAS_GELU_ACT, NONE; N = 4096 (320 tiles on 256 workgroups, plain epilogue) reaches the look-ahead kernel's remapped form.

Every destination is filled with NaN bit patterns before every call.  A row of a block that holds a live row must be torch.equal to
the unfiltered call's, in C and in C2 (nothing is re-grouped: one differing element is a bug).  The rows of blocks without a live row
must be exactly zero with the fill and keep their NaN pattern without it, which proves that nothing was written there; large values in
the input rows of those blocks must not change the result, which proves that nothing was read there."""
import numpy as np
import pytest
import torch

from test_gemm_dgrad_rows_gpu import BLK, KS, M, masks

pytestmark = pytest.mark.gpu

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_ACT = 0, 1, 2, 7
QSCALE = 0.125 * 1.4426950408889634


@pytest.fixture(scope="module")
def operands(gpu):
    g = torch.Generator(device="cpu").manual_seed(8765)
    kmax = max(KS)
    return {"x": torch.randn((M, kmax), generator=g).to(gpu).to(torch.bfloat16),
            "w": (torch.randn((4096, kmax), generator=g) * 0.05).to(gpu).to(torch.bfloat16),
            "bias": torch.randn(4096, generator=g).to(gpu)}


def dead_block_rows(live_np, gpu):
    nb = (M + BLK - 1) // BLK
    return torch.from_numpy(np.repeat([not live_np[t * BLK: (t + 1) * BLK].any() for t in range(nb)], BLK)[:M]).to(gpu)


def is_nan_pattern(t):
    return bool((t.view(torch.int16) == -1).all().item())      # 0xFFFF in every element


CASES = [("bias", EPI_BIAS, 2048, 0), ("bias_qscale", EPI_BIAS, 3072, 1024), ("bias_gelu", EPI_BIAS_GELU, 2048, 0),
         ("bias_gelu_act", EPI_BIAS_GELU_ACT, 2048, 0), ("none", EPI_NONE, 2048, 0), ("none_lookahead", EPI_NONE, 4096, 0)]


@pytest.mark.parametrize("name,epilogue,N,qcols", CASES, ids=[c[0] for c in CASES])
def test_fwd_rows_equals_unfiltered(gpu, operands, name, epilogue, N, qcols):
    from item_alignment_amd import _lib, ops
    lib = _lib.load()
    ff = lambda: torch.full((M, N), -1, device=gpu, dtype=torch.int16).view(torch.bfloat16)      # 0xFFFF: a NaN
    bias = operands["bias"][:N].contiguous() if epilogue != EPI_NONE else None
    two = epilogue == EPI_BIAS_GELU
    for K in KS:
        assert lib.ia_gemm_fwd_rows_filters(M, N, K) == 1
        x = operands["x"][:, :K].contiguous()
        w = operands["w"][:N, :K].contiguous()
        if qcols:
            dense = (ops.gemm_qscale(x, w, bias, qcols, QSCALE),)
        else:
            d = ops.gemm(x, w, epilogue=epilogue, bias=bias, out=ff(), pre_out=ff() if two else None)
            dense = d if two else (d,)
        assert all(torch.isfinite(t.float()).all() for t in dense)

        def run(xin, live, fill):
            r = ops.gemm_fwd_rows(xin, w, live, epilogue=epilogue, bias=bias, scaled_cols=qcols, col_scale=QSCALE if qcols else 1.0, fill=fill,
                                  out=ff(), pre_out=ff() if two else None)
            return r if two else (r,)

        for a, b in zip(run(x, None, True), dense):                    # NULL = the unfiltered call
            assert torch.equal(a, b), (K, "no filter")
        for mname, live_np in masks().items():
            live = torch.from_numpy(live_np).to(gpu)
            dead = dead_block_rows(live_np, gpu)
            tag = (K, mname)
            filled, bare = run(x, live, True), run(x, live, False)
            for got, nofill, want in zip(filled, bare, dense):
                assert torch.equal(got[~dead], want[~dead]), tag       # every row of a live block, in C and in C2
                assert torch.equal(nofill[~dead], want[~dead]), tag
                if dead.any():
                    assert got[dead].float().abs().max().item() == 0.0, tag            # the fill: zeros
                    assert is_nan_pattern(nofill[dead]), tag                           # no fill: nothing was written
            if dead.any():                                             # blocks that are dead as a whole are not read
                xp = torch.where(dead[:, None], torch.tensor(1e4, device=gpu, dtype=torch.bfloat16), x).contiguous()
                for a, b in zip(run(xp, live, True), filled):
                    assert torch.equal(a, b), tag
