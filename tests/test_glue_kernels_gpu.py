"""The small input, head and conv-tower kernels through the C ABI against the fp64 references of tests/glue_reference.py, at the
hidden widths, row counts and edges where such kernels go wrong.  The bars are derived, not measured:

  * pure data movement is bit-exact against torch's own fp32 -> bf16 conversion of the reference (`bits`);
  * a bf16 output of fp32 arithmetic obeys, element by element, |got - want| <= 2^-8 |want| + a (`bf16_close`): one bf16 ulp -- half
    for the rounding, half for the fp32 arithmetic in front of it -- plus `a`, the fp32 bound below, for cancellation near zero;
  * an fp32 output that is a sum obeys, element by element, |got - want| <= c 2^-24 S (`sum_close`): S = the fp64 sum of the absolute
    values of the terms, c = the longest sequential chain of roundings in that kernel (per-lane loop trips + 6 for the wave
    reduction + the epilogue operations), read off the kernel and stated beside each use.

Where the bound is zero (a padded channel, a row outside every span) the output has to be exactly zero.  Every helper prints the
largest error it saw as a fraction of its bound (`-s` shows them); that figure is recorded, never used to set a bound.
"""
import math

import numpy as np
import pytest
import torch

import glue_reference as R
from fp64_bars import TINY, U24, ULP16, _ratio, bf16_close, bits, sum_close

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ERR_ARG, ERR_WS = -1, -3


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


def st():
    from item_alignment_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what):
    from item_alignment_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def P(t):
    return None if t is None else t.data_ptr()


_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    _KEEP.clear()


def PG(t):
    """pointer of a device copy of a host tensor (None -> NULL); the copy lives until the test ends -- launches are asynchronous, and a
    temporary freed right after its pointer was taken would be handed to the next allocation"""
    if t is None:
        return None
    _KEEP.append(t.to("cuda"))
    return _KEEP[-1].data_ptr()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype)


def nv_of(H):
    return (H + 511) // 512


# =============================================================================================================== refusals
def _refusal_cases(p, ws_embed, ws_ln, ws_gap):
    """(entry point, valid tiny argument list, [(changes {index: value}, expected code)]).  p = a zeroed device buffer that is larger
    than anything the tiny valid extents could touch; every change below is one the C code rejects in front of its first launch."""
    s = None   # stream: the default (NULL) stream
    return [
        ("ia_embed_ln_fwd", [p] * 14 + [1, 8, 1e-5, 0.0, 0, 0, s],
         [({0: None}, ERR_ARG), ({13: None}, ERR_ARG), ({14: 0}, ERR_ARG), ({15: 0}, ERR_ARG), ({15: -8}, ERR_ARG), ({15: 12}, ERR_ARG),
          ({15: 4104}, ERR_ARG), ({7: None}, ERR_ARG)]),
        ("ia_embed_ln_bwd", [p] * 19 + [1, 8, 1, -1, -1, 0.0, 0, 0, p, ws_embed, s],
         [({0: None}, ERR_ARG), ({10: None}, ERR_ARG), ({19: 0}, ERR_ARG), ({20: 0}, ERR_ARG), ({20: -8}, ERR_ARG), ({20: 12}, ERR_ARG),
          ({20: 4104}, ERR_ARG), ({28: ws_embed - 1}, ERR_WS), ({27: None}, ERR_WS)]),
        ("ia_im2col_patch", [p, p, 1, 1, 8, 8, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({4: 12, 5: 12}, ERR_ARG),
          ({4: 20}, ERR_ARG)]),
        ("ia_vit_tokens_fwd", [p, p, p, p, 1, 1, 8, s],
         [({0: None}, ERR_ARG), ({3: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({6: -8}, ERR_ARG),
          ({6: 12}, ERR_ARG)]),
        ("ia_vit_tokens_bwd", [p, p, p, p, 1, 1, 8, 0, s],
         [({0: None}, ERR_ARG), ({2: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({6: -8}, ERR_ARG),
          ({6: 12}, ERR_ARG)]),
        ("ia_gather_rows_fwd", [p, 8, p, p, 1, 8, 0.0, 0, 0, s], [({0: None}, ERR_ARG), ({2: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG)]),
        ("ia_gather_rows_bwd", [p, 8, p, p, 1, 8, 0.0, 0, 0, 0, s], [({0: None}, ERR_ARG), ({3: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: -1}, ERR_ARG)]),
        ("ia_pair_head_ce_fwd", [p, p, p, p, p, p, p, p, p, 1, 8, 2, s],
         [({0: None}, ERR_ARG), ({5: None}, ERR_ARG), ({9: 0}, ERR_ARG), ({10: 0}, ERR_ARG), ({11: 0}, ERR_ARG), ({11: 9}, ERR_ARG),
          ({7: None}, ERR_ARG), ({8: None}, ERR_ARG)]),
        ("ia_pair_head_ce_bwd", [p, p, p, p, p, p, p, p, p, p, 1, 8, 2, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: None}, ERR_ARG), ({6: None}, ERR_ARG), ({7: None}, ERR_ARG), ({10: 0}, ERR_ARG),
          ({12: 9}, ERR_ARG)]),
        ("ia_span_mean_fwd", [p, 8, p, p, 1, 8, s],
         [({0: None}, ERR_ARG), ({2: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({5: -8}, ERR_ARG), ({5: 12}, ERR_ARG), ({1: 12}, ERR_ARG)]),
        ("ia_span_mean_bwd", [p, p, p, p, 1, 1, 8, s],
         [({0: None}, ERR_ARG), ({2: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({6: -8}, ERR_ARG), ({6: 12}, ERR_ARG)]),
        ("ia_kg_gather_fwd", [p, p, p, 2, 0, 1, p, p, 1, 1, 4, s],
         [({0: None}, ERR_ARG), ({6: None}, ERR_ARG), ({8: 0}, ERR_ARG), ({9: 0}, ERR_ARG), ({10: 0}, ERR_ARG), ({10: 6}, ERR_ARG)]),
        ("ia_kg_gather_bwd", [p, p, 2, 1, p, 1, 1, 4, s], [({0: None}, ERR_ARG), ({4: None}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({7: 0}, ERR_ARG)]),
        ("ia_kg_rows_fwd", [p, p, p, p, 4, 1, 1, 1, 4, s],
         [({0: None}, ERR_ARG), ({3: None}, ERR_ARG), ({6: 0}, ERR_ARG), ({7: 0}, ERR_ARG), ({8: 0}, ERR_ARG), ({8: 6}, ERR_ARG), ({5: -1}, ERR_ARG),
          ({5: 3}, ERR_ARG), ({4: 2}, ERR_ARG)]),
        ("ia_kg_rows_bwd", [p, 4, 1, p, p, p, 1, 1, 4, s],
         [({0: None}, ERR_ARG), ({5: None}, ERR_ARG), ({6: 0}, ERR_ARG), ({7: 0}, ERR_ARG), ({8: 0}, ERR_ARG), ({2: -1}, ERR_ARG), ({2: 3}, ERR_ARG)]),
        ("ia_pair_sim_fwd", [p, p, p, p, 1, 4, 0, s],
         [({0: None}, ERR_ARG), ({3: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 4}, ERR_ARG), ({6: -1}, ERR_ARG)]),
        ("ia_pair_sim_bwd", [p, p, p, p, p, p, p, p, 1, 4, 0, s],
         [({0: None}, ERR_ARG), ({2: None}, ERR_ARG), ({6: None}, ERR_ARG), ({7: None}, ERR_ARG), ({8: 0}, ERR_ARG), ({9: 0}, ERR_ARG), ({10: 4}, ERR_ARG)]),
        ("ia_nchw_to_nhwc_bf16", [p, p, 1, 3, 2, 2, 8, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 2}, ERR_ARG)]),
        ("ia_ws_conv_weight_fwd", [p, p, p, p, p, 1, 3, 9, 8, 1.0, 1e-5, s],
         [({0: None}, ERR_ARG), ({4: None}, ERR_ARG), ({5: 0}, ERR_ARG), ({6: 0}, ERR_ARG), ({7: 0}, ERR_ARG), ({8: 2}, ERR_ARG)]),
        ("ia_ws_conv_weight_bwd", [p, p, p, p, p, p, p, 1, 3, 9, 8, 1.0, s],
         [({0: None}, ERR_ARG), ({4: None}, ERR_ARG), ({7: 0}, ERR_ARG), ({8: 0}, ERR_ARG), ({9: 0}, ERR_ARG), ({10: 2}, ERR_ARG)]),
        ("ia_silu_fwd", [p, p, 8, 1.0, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({2: 12}, ERR_ARG)]),
        ("ia_silu_bwd", [p, p, p, p, 8, 1.0, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({3: None}, ERR_ARG), ({4: 0}, ERR_ARG), ({4: 12}, ERR_ARG)]),
        ("ia_silu_bwd_sum", [p, p, p, p, p, 8, 1.0, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({4: None}, ERR_ARG), ({5: 0}, ERR_ARG), ({5: 12}, ERR_ARG)]),
        ("ia_avgpool2_fwd", [p, p, 1, 2, 2, 8, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({5: 12}, ERR_ARG)]),
        ("ia_avgpool2_bwd", [p, p, 1, 2, 2, 8, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 0}, ERR_ARG), ({5: 12}, ERR_ARG)]),
        ("ia_gap_fwd", [p, p, 1, 4, 8, p, ws_gap, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 12}, ERR_ARG), ({6: ws_gap - 1}, ERR_WS), ({5: None}, ERR_WS)]),
        ("ia_gap_bwd", [p, p, 1, 4, 8, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 12}, ERR_ARG)]),
        ("ia_pad_rows", [p, p, 1, 2, 2, 8, 0, 1, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({5: 12}, ERR_ARG)]),
        ("ia_conv_weight_pack", [p, p, 1, 3, 9, 8, 72, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 2}, ERR_ARG), ({6: 71}, ERR_ARG)]),
        ("ia_conv_weight_unpack_grad", [p, p, 1, 3, 9, 8, 72, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({5: 2}, ERR_ARG), ({6: 71}, ERR_ARG)]),
        ("ia_ln_bwd2", [p] * 12 + [1, 8, 0.0, 0, 0, p, ws_ln, 0, s],
         [({0: None}, ERR_ARG), ({7: None}, ERR_ARG), ({12: 0}, ERR_ARG), ({13: 0}, ERR_ARG), ({13: -8}, ERR_ARG), ({13: 12}, ERR_ARG), ({13: 4104}, ERR_ARG),
          ({18: ws_ln - 1}, ERR_WS), ({17: None}, ERR_WS), ({8: None, 14: 0.1}, ERR_ARG)]),
        ("ia_ln_bwd2_rows", [p] * 12 + [1, 8, 0.0, 0, 0, p, p, ws_ln, 0, s],
         [({0: None}, ERR_ARG), ({12: 0}, ERR_ARG), ({13: 0}, ERR_ARG), ({13: 12}, ERR_ARG), ({19: ws_ln - 1}, ERR_WS), ({18: None}, ERR_WS)]),
        ("ia_transpose_bf16_batched", [p, p, p, 1, 1, s],
         [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: None}, ERR_ARG), ({3: 0}, ERR_ARG), ({4: 0}, ERR_ARG), ({3: 65536}, ERR_ARG)]),
        ("ia_cast_f32_to_bf16", [p, p, 8, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG)]),
        ("ia_cast_bf16_to_f32", [p, p, 8, s], [({0: None}, ERR_ARG), ({1: None}, ERR_ARG), ({2: 0}, ERR_ARG)]),
    ]


def test_every_documented_precondition_is_refused_before_any_launch(gpu, lib):
    """One call per documented precondition of every entry point of this file: a null required pointer, a non-positive extent, a
    misaligned H / C / Dk / n, Cp < C, row0 + 2P > rows_per_item, more than 8 classes, a workspace one byte short.  Each returns its
    documented code, and the buffer every pointer argument points at -- zeroed, and far larger than the tiny valid extents -- is
    still all zero afterwards: nothing was launched.  H = 0 and H = -8 pass an (H & 7) test; the embedding, ViT-token and LayerNorm
    backward guards used to let them through."""
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    cases = _refusal_cases(buf.data_ptr(), lib.ia_embed_ln_bwd_workspace_bytes(1, 8), lib.ia_ln_bwd_workspace_bytes(1, 8),
                           lib.ia_gap_workspace_bytes(1, 4, 8))
    assert lib.ia_embed_ln_bwd_workspace_bytes(1, 8) <= buf.numel()
    n = 0
    for name, base, bad in cases:
        fn = getattr(lib, name)
        assert len(base) == len(fn.argtypes), name
        for change, code in bad:
            args = list(base)
            for i, v in change.items():
                args[i] = v
            assert fn(*args) == code, (name, change, code)
            n += 1
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0
    print(f"[glue] refusals: {n} calls over {len(cases)} entry points")


# =============================================================================================================== embeddings
def _embed_inputs(M, H, seed, L=None):
    """ids with padding ids, token type 1, a few rows redirected to `extra` rows; tables in fp32"""
    V, T, NP, E, word_pad, pos_pad = 50, 2, 40, 6, 1, 1
    g = gen(seed)
    ids = torch.randint(2, V, (M,), generator=g)
    tts = (torch.rand(M, generator=g) < 0.3).long()
    if L:
        pids = (torch.arange(M) % L) + 2
    else:
        pids = torch.randint(2, NP, (M,), generator=g)
    padrow = torch.rand(M, generator=g) < 0.15
    ids[padrow], pids[padrow] = word_pad, pos_pad
    xi = torch.full((M,), -1, dtype=torch.int32)
    if M >= 8:
        xi[torch.randperm(M, generator=g)[:min(E, M // 4)]] = torch.arange(min(E, M // 4), dtype=torch.int32)
    tabs = dict(word=randn((V, H), seed + 1), type=randn((T, H), seed + 2, 0.5), pos=randn((NP, H), seed + 3, 0.5), extra=randn((E, H), seed + 4))
    tabs["word"][word_pad] = 0
    tabs["pos"][pos_pad] = 0
    gamma, beta = torch.rand(H, generator=g) + 0.5, randn((H,), seed + 5, 0.3)
    return dict(ids=ids, tts=tts, pids=pids, xi=xi, gamma=gamma, beta=beta, **tabs), (V, T, NP, E, word_pad, pos_pad)


def _embed_fwd(lib, dev, M, H, eps, p, seed, sid):
    z, y = torch.empty((M, H), device="cuda", dtype=BF16), torch.empty((M, H), device="cuda", dtype=BF16)
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ok(lib.ia_embed_ln_fwd(P(dev["ids"]), P(dev["tts"]), P(dev["pids"]), P(dev["xi"]), P(dev["word"]), P(dev["type"]), P(dev["pos"]), P(dev["extra"]),
                           P(dev["gamma"]), P(dev["beta"]), P(z), P(y), P(mean), P(rstd), M, H, eps, p, seed, sid, st()), "ia_embed_ln_fwd")
    return z, y, mean, rstd


@pytest.mark.parametrize("M,H", [(37, 8), (37, 64), (37, 504), (37, 512), (37, 520), (37, 768), (1, 768), (37, 1024), (37, 1536), (37, 2048),
                                 (37, 4096), (1, 4096)])
def test_embed_ln_fwd_every_register_chunk(gpu, lib, M, H):
    """ia_embed_ln_fwd over the NV template: one chunk (8, 64, 504, 512), the chunk boundary (520), NV = 2, 3, 4 and the `default: 8`
    arm (4096); 37 rows = nine blocks of 4 waves and one wave over, and a single row.  Word rows mixed with redirected extra rows,
    padding ids, token type 1.  z_out against the fp64 sum; mean, rstd and y against the fp64 LayerNorm of the z the kernel wrote
    (the statistics are documented as those of the rounded z); then dropout 0.1: zeros exactly where the host replica of the hash
    puts them, kept values = the undropped run times inv_keep, z / mean / rstd unchanged."""
    eps = 1e-5
    inp, _ = _embed_inputs(M, H, 100 + H)
    dev = {k: v.to(gpu) for k, v in inp.items()}
    z, y, mean, rstd = _embed_fwd(lib, dev, M, H, eps, 0.0, 0, 0)
    tag = f"embed_fwd[{M}x{H}]"
    # z = bf16((a + b) + c): two fp32 additions -> a = 2 * 2^-24 * (|a| + |b| + |c|)
    zabs = R.embed_sum(inp["ids"], inp["tts"], inp["pids"], inp["xi"], inp["word"].abs(), inp["type"].abs(), inp["pos"].abs(), inp["extra"].abs())
    bf16_close(tag + " z", z, R.embed_sum(inp["ids"], inp["tts"], inp["pids"], inp["xi"], inp["word"], inp["type"], inp["pos"], inp["extra"]),
               2 * U24 * zabs)
    zg = z.cpu().to(F64)
    y64, mean64, rstd64 = R.layernorm_fwd(zg, inp["gamma"], inp["beta"], eps)
    A = zg.abs().mean(1)
    # mean: NV * 8 additions per lane, 6 steps of the wave reduction, one division
    c_m = nv_of(H) * 8 + 6 + 1
    sum_close(tag + " mean", mean, mean64, A, c_m)
    # rstd = rsqrt(sum d^2 / H + eps): all terms positive, so S = var + eps; per lane NV * 8 additions of terms that carry a
    # subtraction and a square, 6 reduction steps, the division and the + eps: c_q; the mean's own error enters squared (sum d = 0);
    # rsqrt halves the relative error of its argument and adds its own ulp (2 * 2^-24) and the final rounding
    c_q = nv_of(H) * 8 + 2 + 6 + 2
    var_eps = 1.0 / rstd64 ** 2
    rel = U24 * (0.5 * c_q + 3) + 0.5 * (c_m * U24 * A) ** 2 / var_eps
    r = _ratio(tag + " rstd", (rstd.cpu().to(F64) - rstd64).abs(), rel * rstd64)
    assert r <= 1.0, (tag, "rstd", r)
    # y = bf16((z - mean) * rstd * gamma + beta): fp32 error of the product <= (c_m + c_q + 8) * 2^-24 of the magnitudes involved
    S = (((zg - mean64[:, None]).abs() + A[:, None]) * rstd64[:, None]) * inp["gamma"].to(F64).abs() + inp["beta"].to(F64).abs()
    bf16_close(tag + " y", y, y64, (c_m + c_q + 8) * U24 * S)

    for p, seed, sid in ((0.1, 1234, 0), (0.1, 77, 3)):
        zd, yd, md, rd = _embed_fwd(lib, dev, M, H, eps, p, seed, sid)
        bits(tag + " z under dropout", zd, z), bits(tag + " mean under dropout", md, mean), bits(tag + " rstd under dropout", rd, rstd)
        keep = R.keep_mask(seed, sid, M * H, p).reshape(M, H)
        _, inv_keep = R.drop_params(p)
        y0, ydc = y.cpu().to(F64), yd.cpu().to(F64)
        assert (ydc[~keep] == 0).all(), (tag, "a dropped element is not zero")
        assert ((ydc != 0) == (y0 != 0))[keep].all(), (tag, "a kept element was zeroed")
        # both runs round the same fp32 value to bf16, times inv_keep in the dropout run: the usual bar for the rounding of the dropout
        # run, and in `a` the rounding the undropped run made (2^-8), the multiplication, and the second-order term 2^-15
        want = y0 * inv_keep
        bf16_close(tag + f" kept values (seed {seed})", yd.cpu()[keep], want[keep], (ULP16 + 2 * U24 + 2.0 ** -15) * want[keep].abs())
        if M * H >= 20000:
            q = R.drop_params(p)[0] / 65536
            assert abs(int(keep.sum()) - M * H * (1 - q)) <= 5 * math.sqrt(M * H * q * (1 - q))


def _embed_bwd_chain(M, L, ordered):
    """(rows one wave walks, workgroups) of embed_ln_bwd_kernel: the grid of embed_bwd_grid / the row_order branch of ia_embed_ln_bwd"""
    if ordered:
        Lc = min(M, 2048)
        S = (M + Lc - 1) // Lc
        gx, gy = min(512, (Lc + 3) // 4), 1
    else:
        if L <= 0 or M % L:
            L = M
        Lc, S = L, M // L
        gx = min(512, (Lc + 3) // 4)
        gy = min(S, max(1, 8192 // (gx * 4)))
    return ((Lc + gx * 4 - 1) // (gx * 4)) * ((S + gy - 1) // gy), gx * gy


@pytest.mark.parametrize("name,M,L,H,ordered,p", [("grid H=768", 117, 13, 768, False, 0.0), ("grid H=1536 dropout", 117, 13, 1536, False, 0.1),
                                                  ("grid H=520", 36, 9, 520, False, 0.0), ("grid H=4096 dropout", 20, 5, 4096, False, 0.1),
                                                  ("row_order M=1001", 1001, 0, 768, True, 0.0),
                                                  ("row_order M=2500 dropout", 2500, 0, 768, True, 0.1),
                                                  ("row_order M=2051 H=1536", 2051, 0, 1536, True, 0.0)])
def test_embed_ln_bwd_all_outputs(gpu, lib, name, M, L, H, ordered, p):
    """ia_embed_ln_bwd: dgamma, dbeta, dextra and the three tables against fp64, every output accumulating onto a non-zero start;
    the [S, L] grid path and the row_order path (a position-sorted list over unpadded rows: M below 2048, above it, and no multiple
    of the 2048 chunks); dropout 0.1 with the forward's mask (the host replica's); H above 512.  Two calls repeat the table
    gradients bit for bit."""
    from item_alignment_amd.models.functional import embed_table_orders
    inp, (V, T, NP, E, word_pad, pos_pad) = _embed_inputs(M, H, 300 + M + H, L=L if not ordered else 29)
    seed, sid = 20240229, 11
    z = randn((M, H), 7, 2.0, BF16)
    dy = randn((M, H), 8, 1.0, BF16)
    zf = z.to(F64)
    mean = zf.mean(1).to(F32)
    rstd = (1.0 / torch.sqrt(zf.var(1, unbiased=False) + 1e-5)).to(F32)
    keep = R.keep_mask(seed, sid, M * H, p).reshape(M, H) if p else torch.ones(M, H, dtype=torch.bool)
    inv_keep = R.drop_params(p)[1]
    dy_eff = dy.to(F64) * keep * inv_keep
    dz, dgamma, dbeta = R.layernorm_bwd(dy_eff, z, mean, rstd, inp["gamma"])
    want = R.embed_table_grads(dz, inp["ids"], inp["tts"], inp["pids"], inp["xi"], V, T, NP, E, word_pad, pos_pad)
    # error scales: the same backward on absolute values
    gam = inp["gamma"].to(F64)
    xh = (zf - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]
    ga = (dy_eff * gam).abs()
    S_row = rstd.to(F64)[:, None] * (ga + ga.mean(1, keepdim=True) + xh.abs() * (ga * xh.abs()).mean(1, keepdim=True))
    S_tab = R.embed_table_grads(S_row, inp["ids"], inp["tts"], inp["pids"], inp["xi"], V, T, NP, E, word_pad, pos_pad)

    dev = {k: v.to(gpu) for k, v in dict(z=z, dy=dy, mean=mean, rstd=rstd, **inp).items()}
    orders = embed_table_orders(dev["ids"], dev["tts"], dev["pids"], dev["xi"], word_pad, pos_pad)
    row_order = torch.argsort(dev["pids"], stable=True).to(torch.int32) if ordered else None
    ws_bytes = lib.ia_embed_ln_bwd_workspace_bytes(M, H)
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)
    init = dict(word=0.25, type=-0.5, pos=0.125, extra=0.75, dgamma=1.5, dbeta=-2.0)

    def run():
        out = {k: torch.full(s, init[k], device=gpu) for k, s in dict(word=(V, H), type=(T, H), pos=(NP, H), extra=(E, H), dgamma=(H,), dbeta=(H,)).items()}
        ok(lib.ia_embed_ln_bwd(P(dev["dy"]), P(dev["z"]), P(dev["mean"]), P(dev["rstd"]), P(dev["gamma"]), P(dev["ids"]), P(dev["tts"]), P(dev["pids"]),
                               P(dev["xi"]), P(row_order), *(P(o) for o in orders), P(out["word"]), P(out["type"]), P(out["pos"]), P(out["extra"]),
                               P(out["dgamma"]), P(out["dbeta"]), M, H, L, word_pad, pos_pad, p, seed, sid, P(ws), ws_bytes, st()), "ia_embed_ln_bwd")
        return out

    g1, g2 = run(), run()
    for k in ("word", "type", "pos"):
        bits(f"embed_bwd[{name}] {k} table, second call", g2[k], g1[k])
    # one row's input gradient: NV * 8 products per lane and 6 reduction steps for each of the two row means, ten element-wise operations
    c_row = nv_of(H) * 8 + 6 + 10
    pieces = (M + 511) // 512
    for k in ("word", "type", "pos"):
        # a table row: its rows summed in pieces of 512 sorted positions (a chain of up to 512), the pieces joined in order, onto the start
        sum_close(f"embed_bwd[{name}] d{k}", g1[k], want[k] + init[k], S_tab[k] + abs(init[k]), c_row + 512 + pieces + 2)
    assert g1["word"].cpu()[word_pad].eq(init["word"]).all() and g1["pos"].cpu()[pos_pad].eq(init["pos"]).all()
    # dextra: one fp32 atomic per redirected row onto the start
    sum_close(f"embed_bwd[{name}] dextra", g1["extra"], want["extra"] + init["extra"], S_tab["extra"] + abs(init["extra"]), c_row + 2)
    # dgamma / dbeta: a wave's chain over the rows it walks, 3 additions across the block's waves, the second stage's chain over
    # workgroups (ceil(nb / 32) + 32) and the accumulation; 4 operations inside a term (xhat, the product, the dropout scale)
    chain, nb = _embed_bwd_chain(M, L, ordered)
    c_g = chain + 3 + (nb + 31) // 32 + 32 + 1 + 4
    sum_close(f"embed_bwd[{name}] dgamma", g1["dgamma"], dgamma + init["dgamma"], (dy_eff * xh).abs().sum(0) + abs(init["dgamma"]), c_g)
    sum_close(f"embed_bwd[{name}] dbeta", g1["dbeta"], dbeta + init["dbeta"], dy_eff.abs().sum(0) + abs(init["dbeta"]), c_g)


# =============================================================================================================== ViT input side
@pytest.mark.parametrize("B,C,S,Pp", [(2, 3, 32, 16), (1, 3, 48, 8), (3, 1, 16, 16)])
def test_im2col_patch_is_a_bit_exact_gather(gpu, lib, B, C, S, Pp):
    img = randn((B, C, S, S), 1)
    out = torch.full((B * (S // Pp) ** 2, C * Pp * Pp), 7.0, device=gpu, dtype=BF16)
    ok(lib.ia_im2col_patch(PG(img), P(out), B, C, S, Pp, st()), "ia_im2col_patch")
    bits("im2col_patch", out, R.im2col_patch(img, Pp))


@pytest.mark.parametrize("B,NP,H", [(3, 5, 8), (2, 4, 768), (5, 3, 1024)])
def test_vit_tokens_fwd_bwd(gpu, lib, B, NP, H):
    patch, cls, pos = randn((B, NP, H), 1, 1.0, BF16), randn((H,), 2), randn((NP + 1, H), 3)
    tok = torch.empty((B, NP + 1, H), device=gpu, dtype=BF16)
    ok(lib.ia_vit_tokens_fwd(PG(patch), PG(cls), PG(pos), P(tok), B, NP, H, st()), "ia_vit_tokens_fwd")
    # one fp32 addition in front of the rounding
    bf16_close(f"vit_tokens_fwd[{B}x{NP}x{H}]", tok, R.vit_tokens(patch, cls, pos), U24 * R.vit_tokens(patch.abs(), cls.abs(), pos.abs()))
    dtok = randn((B, NP + 1, H), 4, 1.0, BF16)
    dpatch64, dcls64, dpos64 = R.vit_tokens_bwd(dtok)
    _, Scls, Spos = R.vit_tokens_bwd(dtok.abs())
    for acc, start in ((0, float("nan")), (1, 0.5)):
        dpatch = torch.zeros((B, NP, H), device=gpu, dtype=BF16)
        dcls, dpos = torch.full((H,), start, device=gpu), torch.full((NP + 1, H), start, device=gpu)
        ok(lib.ia_vit_tokens_bwd(PG(dtok), P(dpatch), P(dcls), P(dpos), B, NP, H, acc, st()), "ia_vit_tokens_bwd")
        bits("vit_tokens_bwd dpatch", dpatch, dpatch64)
        add = start if acc else 0.0
        # B additions down the batch, one more onto the start
        sum_close(f"vit_tokens_bwd[{B}x{NP}x{H}, accumulate {acc}] dpos", dpos, dpos64 + add, Spos + abs(add), B + 1)
        sum_close(f"vit_tokens_bwd[{B}x{NP}x{H}, accumulate {acc}] dcls", dcls, dcls64 + add, Scls + abs(add), B + 1)


@pytest.mark.parametrize("B,H,ld", [(5, 7, 16), (3, 768, 800), (1, 1, 8), (67, 65, 65)])
def test_gather_rows_fwd_bwd_share_one_mask(gpu, lib, B, H, ld):
    """ia_gather_rows: ld > H, odd H (a hash pair straddles two rows), no dropout (a bit-exact widening copy) and dropout 0.1, where
    forward and backward both zero exactly the elements the host replica names and scale the rest by inv_keep in fp32; accumulate
    0 and 1; rows and columns outside the gather keep their contents."""
    nrows = 3 * B + 2
    src = randn((nrows, ld), 1, 1.0, BF16)
    rows = torch.randperm(nrows, generator=gen(2))[:B].to(torch.int32)
    dout = randn((B, H), 3)
    for p, seed, sid in ((0.0, 0, 0), (0.1, 5, 1), (0.5, 77, 3)):
        keep = R.keep_mask(seed, sid, B * H, p).reshape(B, H) if p else torch.ones(B, H, dtype=torch.bool)
        inv = torch.tensor(R.drop_params(p)[1], dtype=F32)
        out = torch.full((B, H), 9.0, device=gpu)
        ok(lib.ia_gather_rows_fwd(PG(src), ld, PG(rows), P(out), B, H, p, seed, sid, st()), "ia_gather_rows_fwd")
        picked = src[rows.long()][:, :H].to(F32)
        bits(f"gather_rows_fwd[p={p}]", out, torch.where(keep, picked * inv if p else picked, torch.zeros(())))
        for acc in (0, 1):
            dsrc0 = randn((nrows, ld), 4, 1.0, BF16)
            dsrc = dsrc0.to(gpu)
            ok(lib.ia_gather_rows_bwd(PG(dout), ld, PG(rows), P(dsrc), B, H, p, seed, sid, acc, st()), "ia_gather_rows_bwd")
            v = torch.where(keep, dout * inv if p else dout, torch.zeros(()))
            want = dsrc0.clone()
            want[rows.long(), :H] = ((dsrc0[rows.long(), :H].to(F32) + v) if acc else v).to(BF16)      # one fp32 addition, one rounding
            if p and acc:      # old + dout * inv_keep may be contracted into one fused operation: the bf16 bar on the written rows
                old = dsrc0[rows.long(), :H].to(F64)
                bf16_close(f"gather_rows_bwd[p={p}, accumulate]", dsrc.cpu()[rows.long(), :H], old + v.to(F64), 2 * U24 * (old.abs() + v.to(F64).abs()))
                assert ((dsrc.cpu()[rows.long(), :H] == dsrc0[rows.long(), :H]) | keep).all(), "a dropped element changed its row"
                got = dsrc.cpu().clone()
                got[rows.long(), :H] = want[rows.long(), :H]
                bits(f"gather_rows_bwd[p={p}, accumulate] outside the gather", got, want)
            else:
                bits(f"gather_rows_bwd[p={p}, accumulate {acc}]", dsrc, want)


# =============================================================================================================== heads
@pytest.mark.parametrize("H,ld", [(8, 16), (768, 776), (1024, 1024)])
def test_span_mean_fwd_bwd(gpu, lib, H, ld):
    """Spans of length 1 and of length L, two overlapping spans in one sample, a sample without spans, rows outside every span, ld > H."""
    B, L = 4, 7
    seq = randn((B * L, ld), 1, 1.0, BF16)
    spans = torch.tensor([[0, 1], [2, 6], [4, 7], [14, 21], [21, 22], [22, 28]], dtype=torch.int32)     # sample 1 has none
    span_ptr = torch.tensor([0, 3, 3, 4, 6], dtype=torch.int32)
    S = spans.shape[0]
    out = torch.empty((S, H), device=gpu)
    ok(lib.ia_span_mean_fwd(PG(seq), ld, PG(spans), P(out), S, H, st()), "ia_span_mean_fwd")
    # a chain of len additions, the reciprocal and the product; S = mean |row|
    sum_close(f"span_mean_fwd[H={H}]", out, R.span_mean(seq[:, :H], spans), R.span_mean(seq[:, :H].abs(), spans), L + 2)
    dout = randn((S, H), 2)
    dseq = torch.full((B * L, H), 5.0, device=gpu, dtype=BF16)
    ok(lib.ia_span_mean_bwd(PG(dout), PG(spans), PG(span_ptr), P(dseq), B, L, H, st()), "ia_span_mean_bwd")
    want = R.span_mean_bwd(dout, spans, B * L)
    # per span a reciprocal, a product and an addition; at most 3 spans per sample
    bf16_close(f"span_mean_bwd[H={H}]", dseq, want, 9 * U24 * R.span_mean_bwd(dout.abs(), spans, B * L))
    got = dseq.cpu().to(F64)
    assert (got[L:2 * L] == 0).all() and (got[1] == 0).all()          # the sample without spans, a row outside every span
    assert (want[4:6] != R.span_mean_bwd(dout[1:2], spans[1:2], B * L)[4:6]).any()      # rows 4, 5 lie in two spans


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("B", [1, 67])
@pytest.mark.parametrize("D", [40, 768, 1000])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_pair_head_ce_fwd_bwd(gpu, lib, C, D, B, two):
    """ia_pair_head_ce: 2, 3 and 8 classes; D below 64 and no multiple of 64; one- and two-feature forms; B = 1 and 67; the first two
    rows are scaled to logits of +-80 (the max-subtraction); labels NULL in the forward; dW / db accumulate."""
    F = 2 * D if two else D
    x, y = randn((B, D), 1), (randn((B, D), 2) if two else None)
    W, bias = randn((C, F), 3, 0.1), randn((C,), 4, 0.1)
    x[0] = 80.0 * W[0, :D] / (W[0, :D] ** 2).sum()
    if two:
        y[0] = 0
    if B > 1:
        x[1] = -x[0]
        if two:
            y[1] = 0
    labels = torch.randint(0, C, (B,), generator=gen(5))
    dv = lambda t: None if t is None else t.to(gpu)
    xd, yd, Wd, bd, ld_ = dv(x), dv(y), dv(W), dv(bias), dv(labels)
    tag = f"pair_head[C={C} D={D} B={B} two={two}]"

    def fwd(lab):
        logits, probs = torch.empty((B, C), device=gpu), torch.empty((B, C), device=gpu)
        loss, loss_per = torch.full((1,), -7.0, device=gpu), torch.empty(B, device=gpu)
        ok(lib.ia_pair_head_ce_fwd(P(xd), P(yd), P(Wd), P(bd), P(lab), P(logits), P(probs), P(loss), P(loss_per), B, D, C, st()), "ia_pair_head_ce_fwd")
        return logits, probs, loss

    logits, probs, loss = fwd(ld_)
    l0, p0, loss0 = fwd(None)
    bits(tag + " logits without labels", l0, logits), bits(tag + " probs without labels", p0, probs)
    assert loss0.item() == -7.0, "loss is written although labels is NULL"
    lg64, _, _ = R.pair_head_ce(x, y, W, bias, None)
    Slg, _, _ = R.pair_head_ce(x.abs(), None if y is None else y.abs(), W.abs(), bias.abs(), None)
    # per lane ceil(D / 64) products (twice for two features), 6 reduction steps, the bias; one rounding inside each product
    c_lg = (D + 63) // 64 * (2 if two else 1) + 6 + 1 + 1
    sum_close(tag + " logits", logits, lg64, Slg, c_lg)
    assert lg64[0, 0] > 75 and (B == 1 or lg64[1, 0] < -75)
    # softmax / CE of the logits the kernel produced: exp(lg - mx) is good to (|lg - mx| + 3) * 2^-24 (the subtraction's rounding
    # scales with the argument), the denominator adds C roundings, the quotient one
    lgg = logits.cpu().to(F64)
    _, pr64, _ = R.pair_head_ce(lgg, None, torch.eye(C, dtype=F64), None, None)
    dlt = (lgg.max(1, keepdim=True).values - lgg).max(1, keepdim=True).values
    r = _ratio(tag + " probs", (probs.cpu().to(F64) - pr64).abs(), pr64 * U24 * (2 * dlt + 8 + C) + TINY)
    assert r <= 1.0, (tag, "probs", r)
    mx = lgg.max(1).values
    lse = torch.log(torch.exp(lgg - mx[:, None]).sum(1))
    per = lse - (lgg[torch.arange(B), labels] - mx)
    # per sample: two subtractions and logf on magnitudes |lg_l - mx| + |log den|, the denominator's relative error (dlt + C + 3) passes
    # through the log unchanged; the mean is a chain of ceil(B / 64) + 6 + 1
    bound = U24 * ((math.ceil(B / 64) + 7) * per.abs().mean() + (3 * ((lgg[torch.arange(B), labels] - mx).abs() + lse.abs()) + dlt[:, 0] + C + 4).mean())
    r = _ratio(tag + " loss", (loss.cpu().to(F64) - per.mean()).abs().reshape(1), bound.reshape(1))
    assert r <= 1.0, (tag, "loss", r)

    dloss = torch.tensor([0.7])
    dx, dyv = torch.empty((B, D), device=gpu), (torch.empty((B, D), device=gpu) if two else None)
    dW, db = torch.full((C, F), 0.5, device=gpu), torch.full((C,), -0.25, device=gpu)
    ok(lib.ia_pair_head_ce_bwd(P(probs), P(ld_), PG(dloss), P(xd), P(yd), P(Wd), P(dx), P(dyv), P(dW), P(db), B, D, C, st()), "ia_pair_head_ce_bwd")
    pg = probs.cpu()
    dx64, dy64, dW64, db64 = R.pair_head_ce_bwd(pg, labels, dloss.item(), x, y, W)
    onehot = torch.zeros(B, C, dtype=F64)
    onehot[torch.arange(B), labels] = 1.0
    ga = (pg.to(F64) - onehot).abs() * (dloss.item() / B)
    fa = x.abs().to(F64) if not two else torch.cat((x.abs(), y.abs()), 1).to(F64)
    Sdf = ga @ W.abs().to(F64)
    # dx, dy: C terms, each with the one-hot subtraction, the scale (itself a quotient) and the product
    sum_close(tag + " dx", dx, dx64, Sdf[:, :D], C + 4)
    if two:
        sum_close(tag + " dy", dyv, dy64, Sdf[:, D:], C + 4)
    # dW, db: B terms down the batch, the same three operations inside a term, one addition onto the start
    sum_close(tag + " dW", dW, dW64 + 0.5, ga.t() @ fa + 0.5, B + 5)
    sum_close(tag + " db", db, db64 - 0.25, ga.sum(0) + 0.25, B + 5)


# =============================================================================================================== PKGM rows
@pytest.mark.parametrize("B,Pn,Dk", [(5, 3, 8), (3, 10, 200), (1, 1, 4)])
def test_kg_gather_sign_and_relation_scatter(gpu, lib, B, Pn, Dk):
    """ia_kg_gather: entity rows with +0.0, -0.0, denormals and +-1e-30 -- the output is sign(x) with sign(+-0) = +0.0 (bit pattern
    0x00000000 for -0.0 too); relation rows are copied bit for bit; ids are read at ent_col / rel_lo of rows wider than the columns
    used; relations repeat inside the batch, so the backward's atomics add up to the fp64 scatter within the sum bound."""
    NE, NR, ld_ids, ent_col, rel_lo = 7, 4, Pn + 4, 1, 2
    ent, rel = randn((NE, Dk), 1), randn((NR, Dk), 2)
    ent[:, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    ent[0, :4] = torch.tensor([1e-40, -1e-40, 2.0 ** -149, -2.0 ** -149])          # fp32 denormals
    ids = torch.full((B, ld_ids), 3, dtype=torch.long)                               # the columns outside the ones named (valid ids, never read)
    ids[:, ent_col] = torch.arange(B) % NE
    ids[:, rel_lo:rel_lo + Pn] = torch.randint(0, NR, (B, Pn), generator=gen(3))
    h_sign, r = torch.full((B, Dk), 9.0, device=gpu), torch.full((B * Pn, Dk), 9.0, device=gpu)
    ok(lib.ia_kg_gather_fwd(PG(ent), PG(rel), PG(ids), ld_ids, ent_col, rel_lo, P(h_sign), P(r), B, Pn, Dk, st()), "ia_kg_gather_fwd")
    h64, r64 = R.kg_gather(ent, rel, ids, ent_col, rel_lo, Pn)
    e = ent[ids[:, ent_col]]
    want = torch.where(e > 0, torch.ones(()), torch.where(e < 0, -torch.ones(()), torch.zeros(())))
    assert torch.equal(want.to(F64), h64 + 0.0)
    bits("kg_gather h_sign", h_sign, want)
    assert h_sign.cpu().view(torch.int32)[0, :2].tolist() == ([0x3F800000, -0x40800000] if ids[0, ent_col] == 0 else [0, 0])
    assert (h_sign.cpu().view(torch.int32)[:, :2][ids[:, ent_col] != 0] == 0).all(), "sign(+0.0) and sign(-0.0) must both be +0.0"
    bits("kg_gather r", r, r64)
    dr = randn((B * Pn, Dk), 4)
    grad = torch.full((NR, Dk), 0.5, device=gpu)
    ok(lib.ia_kg_gather_bwd(PG(dr), PG(ids), ld_ids, rel_lo, P(grad), B, Pn, Dk, st()), "ia_kg_gather_bwd")
    # as many atomic additions onto one element as the relation occurs in the batch, in any order
    occ = int(torch.bincount(ids[:, rel_lo:rel_lo + Pn].reshape(-1), minlength=NR).max())
    sum_close(f"kg_gather_bwd[{B}x{Pn}x{Dk}]", grad, R.kg_gather_bwd(dr, ids, rel_lo, Pn, NR) + 0.5, R.kg_gather_bwd(dr.abs(), ids, rel_lo, Pn, NR) + 0.5, occ)


@pytest.mark.parametrize("Pn", [1, 10])
@pytest.mark.parametrize("H", [4, 1024])
def test_kg_rows_window(gpu, lib, Pn, H):
    """ia_kg_rows: row0 > 0 and rows_per_item > row0 + 2P -- rows outside the written window keep a sentinel."""
    B, row0 = 3, 2
    rpi = row0 + 2 * Pn + 3
    h, r, hp = randn((B, H), 1), randn((B * Pn, H), 2), randn((B, H), 3)
    rows = torch.full((B, rpi, H), 777.0, device=gpu)
    ok(lib.ia_kg_rows_fwd(PG(h), PG(r), PG(hp), P(rows), rpi, row0, B, Pn, H, st()), "ia_kg_rows_fwd")
    got = rows.cpu()
    assert (got[:, :row0] == 777.0).all() and (got[:, row0 + 2 * Pn:] == 777.0).all()
    # one fp32 addition per element
    sum_close(f"kg_rows_fwd[P={Pn} H={H}]", got[:, row0:row0 + 2 * Pn], R.kg_rows(h, r, hp),
              torch.cat((h.abs()[:, None] + r.abs().reshape(B, Pn, H), hp.abs()[:, None] + r.abs().reshape(B, Pn, H)), 1), 1)
    g = torch.full((B, rpi, H), float("nan"))
    g[:, row0:row0 + 2 * Pn] = randn((B, 2 * Pn, H), 4)
    dh, dr, dhp = (torch.full(s, 9.0, device=gpu) for s in ((B, H), (B * Pn, H), (B, H)))
    ok(lib.ia_kg_rows_bwd(PG(g), rpi, row0, P(dh), P(dr), P(dhp), B, Pn, H, st()), "ia_kg_rows_bwd")
    win = g[:, row0:row0 + 2 * Pn]
    dh64, dr64, dhp64 = R.kg_rows_bwd(win)
    wa = win.abs()
    # dh, dhp: a chain of P additions; dr: one subtraction
    sum_close(f"kg_rows_bwd[P={Pn} H={H}] dh", dh, dh64, wa[:, :Pn].sum(1), Pn)
    sum_close(f"kg_rows_bwd[P={Pn} H={H}] dhp", dhp, dhp64, wa[:, Pn:].sum(1), Pn)
    sum_close(f"kg_rows_bwd[P={Pn} H={H}] dr", dr, dr64, (wa[:, :Pn] + wa[:, Pn:]).reshape(-1, H), 1)


# =============================================================================================================== similarity head
@pytest.mark.parametrize("measure", [R.SIM_INNER, R.SIM_COSINE, R.SIM_L1, R.SIM_L2])
@pytest.mark.parametrize("D", [3, 64, 200, 1024])
def test_pair_sim_fwd_bwd(gpu, lib, D, measure):
    """ia_pair_sim at D below 64, 64, no multiple of 64 and 1024, each of dsim / dprobs NULL in turn.  Row 5 of x is all zero: every
    output stays finite there, and for cosine sim == 0 and probs == 0.5 (forward clamps |x|^2 |y|^2 at eps^2, backward clamps each
    squared norm at eps: both give zeros, not NaN).  The gradient of that one row of 67 (1.5 % of the elements) is the only thing
    not compared against fp64."""
    B, zr = 67, 5
    x, y = randn((B, D), 10 + D, 0.3), randn((B, D), 20 + D, 0.3)
    x[zr] = 0
    live = torch.arange(B) != zr
    assert ((x - y).to(F64) + R.DIST_EPS).abs().min() > 1e-7          # no difference so close to zero that fp32 could flip its sign
    xd, yd = x.to(gpu), y.to(gpu)
    sim, probs = torch.empty(B, device=gpu), torch.empty(B, device=gpu)
    ok(lib.ia_pair_sim_fwd(P(xd), P(yd), P(sim), P(probs), B, D, measure, st()), "ia_pair_sim_fwd")
    tag = f"pair_sim[measure {measure}, D={D}]"
    x64, y64 = x.to(F64), y.to(F64)
    s64, _ = R.pair_sim(x64, y64, measure)
    c0 = (D + 63) // 64 + 6 + 1          # per-lane chain, wave reduction, one rounding inside a term
    if measure == R.SIM_INNER:
        bound = c0 * U24 * (x64 * y64).abs().sum(1)
    elif measure == R.SIM_COSINE:
        # numerator: c0 on sum |x y|; the two squared norms c0 each, halved by the square root; the product, rsqrt (2) and final product
        nn_ = torch.sqrt(((x64 * x64).sum(1) * (y64 * y64).sum(1)).clamp(min=R.COS_EPS ** 2))
        bound = U24 * (c0 * (x64 * y64).abs().sum(1) / nn_ + s64.abs() * (c0 + 4))
    elif measure == R.SIM_L1:
        bound = (c0 + 2) * U24 * s64                                   # two roundings in u - v + eps
    else:
        bound = U24 * s64 * (0.5 * (c0 + 3) + 2)                      # sqrt halves the sum's relative error, adds its own rounding
    sg = sim.cpu().to(F64)
    r = _ratio(tag + " sim", (sg - s64).abs(), bound)
    assert r <= 1.0, (tag, "sim", r)
    # probs from the sim the kernel wrote; __expf(t) = exp2(t * log2 e) is good to (2 |t| + 3) * 2^-24 relative: the fp32 constant
    # log2 e and the product each put up to 2^-24 |t log2 e| into the exponent, the exp2 and the final rounding add 3
    pg = probs.cpu().to(F64)
    if measure == R.SIM_INNER:
        p64 = torch.sigmoid(sg)
        pb = U24 * ((2 * sg.abs() + 4) * p64 * (1 - p64) + 3 * p64)
    elif measure == R.SIM_COSINE:
        p64, pb = (sg + 1) * 0.5, U24 * (sg.abs() + 1)
    else:
        p64 = torch.exp(-sg)
        pb = U24 * (2 * sg.abs() + 3) * p64 + TINY
    r = _ratio(tag + " probs", (pg - p64).abs(), pb)
    assert r <= 1.0, (tag, "probs", r)
    if measure == R.SIM_COSINE:
        assert sim[zr].item() == 0.0 and probs[zr].item() == 0.5

    dsim, dprobs = randn((B,), 31), randn((B,), 32)
    for ds, dp in ((dsim, dprobs), (dsim, None), (None, dprobs)):
        dx, dyv = torch.full((B, D), float("nan"), device=gpu), torch.full((B, D), float("nan"), device=gpu)
        ok(lib.ia_pair_sim_bwd(P(xd), P(yd), P(sim), P(probs), PG(ds), PG(dp), P(dx), P(dyv),
                               B, D, measure, st()), "ia_pair_sim_bwd")
        assert torch.isfinite(dx).all() and torch.isfinite(dyv).all(), (tag, "non-finite gradient (the all-zero row?)")
        dx64, dy64 = R.pair_sim_bwd(x[live], y[live], None if ds is None else ds[live], None if dp is None else dp[live], measure, sim=sg[live], probs=pg[live])
        xa, ya, sl, pl = x64[live].abs(), y64[live].abs(), sg[live], pg[live]
        dpds = {R.SIM_INNER: pl * (1 - pl), R.SIM_COSINE: torch.full_like(pl, 0.5), R.SIM_L1: pl, R.SIM_L2: pl}[measure]
        G = ((0 if ds is None else ds[live].to(F64).abs()) + (0 if dp is None else dp[live].to(F64).abs() * dpds))[:, None]
        if measure == R.SIM_INNER:
            Sx, Sy, c = G * ya, G * xa, 5                              # g: p (1 - p) (2), product, sum; then the product with the feature
        elif measure == R.SIM_COSINE:
            n1, n2 = (xa * xa).sum(1, keepdim=True), (ya * ya).sum(1, keepdim=True)
            inv = 1.0 / torch.sqrt(n1 * n2)
            Sx, Sy = G * (ya * inv + sl.abs()[:, None] * xa / n1), G * (xa * inv + sl.abs()[:, None] * ya / n2)
            c = c0 + 10                                                # the norms' chains, rsqrt, two products, quotient, difference, g
        elif measure == R.SIM_L1:
            Sx = Sy = G.expand(-1, D)
            c = 3
        else:
            Sx = Sy = G * ((x64[live] - y64[live] + R.DIST_EPS).abs() / sl[:, None])
            c = 8                                                      # d (2), quotient, g (3), product
        names = "both" if ds is not None and dp is not None else ("dsim only" if dp is None else "dprobs only")
        sum_close(tag + f" dx ({names})", dx.cpu()[live], dx64, Sx, c)
        sum_close(tag + f" dy ({names})", dyv.cpu()[live], dy64, Sy, c)


# =============================================================================================================== conv tower pieces
@pytest.mark.parametrize("m,s", [(0.0, 0.02), (0.5, 0.02), (0.5, 0.001)])
@pytest.mark.parametrize("Cout,Cg,kk,Cgp", [(16, 3, 9, 8), (6, 64, 9, 64), (1536, 384, 1, 384), (5, 8, 1, 8)])
def test_ws_conv_weight_fwd_bwd(gpu, lib, Cout, Cg, kk, Cgp, m, s):
    """ia_ws_conv_weight: the stem (3 channels padded to 8: the padded channels are exact zeros), a 64-channel 3x3 group, a wide 1x1
    and a fan-in of 8 (fewer than 64 lanes of work), on weights N(m, s).  The reference is the fp64 two-pass variance and alone sets
    the bars: rstd within 4 * 2^-24 relative, `what` within one bf16 ulp (plus the fp32 term for elements next to the mean).  A
    one-pass E[w^2] - mean^2 in fp32 misses the rstd bar by orders of magnitude at (0.5, 0.001): its variance of 1e-6 is the
    difference of two numbers near 0.25.  dw and dgain accumulate, and each may be NULL."""
    scale, eps = 0.37, 1e-5
    w = (randn((Cout, Cg, kk), 1) * s + m)
    gain = torch.rand(Cout, generator=gen(2)) + 0.5
    what = torch.full((Cout, kk, Cgp), 3.0, device=gpu, dtype=BF16)
    mean, rstd = torch.empty(Cout, device=gpu), torch.empty(Cout, device=gpu)
    wd, gd = w.to(gpu), gain.to(gpu)
    ok(lib.ia_ws_conv_weight_fwd(P(wd), P(gd), P(what), P(mean), P(rstd), Cout, Cg, kk, Cgp, scale, eps, st()), "ia_ws_conv_weight_fwd")
    tag = f"ws_weight[{Cout}x{Cg}x{kk}->{Cgp}, N({m}, {s})]"
    what64, mean64, rstd64 = R.ws_weight(w, gain, scale, eps, Cgp)
    fan = Cg * kk
    c_m = (fan + 63) // 64 + 6 + 1                                     # per-lane chain, wave reduction, the division
    A = w.to(F64).abs().reshape(Cout, -1).mean(1)
    sum_close(tag + " mean", mean, mean64, A, c_m)
    r = _ratio(tag + " rstd", (rstd.cpu().to(F64) - rstd64).abs(), 4 * U24 * rstd64)
    assert r <= 1.0, (tag, "rstd", r)
    # what = bf16((w - mu) * (rstd * gain * scale)): the mean's error (c_m * 2^-24 * A) does not shrink with |w - mu|
    k = (rstd64 * gain.to(F64) * scale)[:, None, None]
    a = torch.zeros_like(what64)
    a[:, :, :Cg] = (U24 * (c_m * A[:, None, None] + 8 * (w.to(F64) - mean64[:, None, None]).abs()) * k).permute(0, 2, 1)
    bf16_close(tag + " what", what, what64, a)
    assert (what.cpu()[:, :, Cg:].view(torch.int16) == 0).all(), "padded channels must be +0.0"

    dwhat = torch.full((Cout, kk, Cgp), float("nan"))                  # the padded channels' gradient is never read
    dwhat[:, :, :Cg] = randn((Cout, kk, Cg), 3)
    mg, rg = mean.cpu(), rstd.cpu()
    dw64, dgain64 = R.ws_weight_bwd(dwhat, w, gain, mg, rg, scale)
    g = dwhat[:, :, :Cg].permute(0, 2, 1).to(F64).abs()
    xh = ((w.to(F64) - mg.to(F64)[:, None, None]) * rg.to(F64)[:, None, None]).abs()
    mga, mgxa = g.reshape(Cout, -1).mean(1)[:, None, None], (g * xh).reshape(Cout, -1).mean(1)[:, None, None]
    Sdw = (gain.to(F64) * scale * rg.to(F64))[:, None, None] * (g + mga + xh * mgxa)
    Sdg = scale * (g * xh).reshape(Cout, -1).sum(1)
    chain = (fan + 63) // 64 + 6
    for use_dw, use_dg in ((True, True), (True, False), (False, True)):
        dw, dgain = torch.full((Cout, Cg, kk), 0.5, device=gpu), torch.full((Cout,), -0.25, device=gpu)
        ok(lib.ia_ws_conv_weight_bwd(PG(dwhat), P(wd), P(gd), P(mean), P(rstd), P(dw if use_dw else None), P(dgain if use_dg else None),
                                     Cout, Cg, kk, Cgp, scale, st()), "ia_ws_conv_weight_bwd")
        if use_dw:     # two row means (chain each), xhat (2), the coefficient (2), three operations in the bracket, product, accumulation
            sum_close(tag + " dw", dw, dw64 + 0.5, Sdw + 0.5, chain + 10)
        else:
            assert (dw == 0.5).all()
        if use_dg:     # the chain, xhat (2), the product, the scale, the accumulation
            sum_close(tag + " dgain", dgain, dgain64 - 0.25, Sdg + 0.25, chain + 5)
        else:
            assert (dgain == -0.25).all()


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("H,W", [(8, 8), (7, 9), (1, 5), (25, 25)])
def test_avgpool2_ceil_mode_edges(gpu, lib, H, W, C):
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False): at an odd edge the window holds 2 or 1 pixels and both directions
    divide by that count.  The backward divides a bf16 value by 1, 2 or 4, which is exact: bit for bit."""
    B = 2
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = randn((B, H, W, C), 1, 1.0, BF16)
    y = torch.empty((B, Ho, Wo, C), device=gpu, dtype=BF16)
    ok(lib.ia_avgpool2_fwd(PG(x), P(y), B, H, W, C, st()), "ia_avgpool2_fwd")
    # up to 3 additions and the division
    bf16_close(f"avgpool2_fwd[{H}x{W}x{C}]", y, R.avgpool2(x), 4 * U24 * R.avgpool2(x.abs()))
    dy = randn((B, Ho, Wo, C), 2, 1.0, BF16)
    dx = torch.empty((B, H, W, C), device=gpu, dtype=BF16)
    ok(lib.ia_avgpool2_bwd(PG(dy), P(dx), B, H, W, C, st()), "ia_avgpool2_bwd")
    bits(f"avgpool2_bwd[{H}x{W}x{C}]", dx, R.avgpool2_bwd(dy, H, W))


def _nsplit(HW):
    return max(1, min(64, HW // 64))


@pytest.mark.parametrize("C", [8, 1536])
@pytest.mark.parametrize("HW", [1, 49, 625, 10000])
def test_gap_fwd_bwd(gpu, lib, HW, C):
    """Global average pool with 1, 1, 9 and 64 slices of HW; 8 channels (256 row lanes per column) and 1536 (one)."""
    B = 2
    x = randn((B, HW, C), 1, 1.0, BF16)
    ws_bytes = lib.ia_gap_workspace_bytes(B, HW, C)
    assert ws_bytes == B * _nsplit(HW) * C * 4
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)
    pooled = torch.empty((B, C), device=gpu)
    xd = x.to(gpu)
    assert lib.ia_gap_fwd(P(xd), P(pooled), B, HW, C, P(ws), ws_bytes - 1, st()) == ERR_WS
    ok(lib.ia_gap_fwd(P(xd), P(pooled), B, HW, C, P(ws), ws_bytes, st()), "ia_gap_fwd")
    ns = _nsplit(HW)
    per = (HW + ns - 1) // ns
    nlane = 256 // min(C // 8, 256)
    # a row lane's chain over its share of the slice, the fold of the row lanes, the chain over the slices, the scale
    c = (per + nlane - 1) // nlane + (nlane - 1) + ns + 1
    sum_close(f"gap_fwd[HW={HW} C={C}]", pooled, R.gap(x), R.gap(x.abs()), c)
    dp = randn((B, C), 2)
    dx = torch.empty((B, HW, C), device=gpu, dtype=BF16)
    ok(lib.ia_gap_bwd(PG(dp), P(dx), B, HW, C, st()), "ia_gap_bwd")
    # the reciprocal of HW and the product
    bf16_close(f"gap_bwd[HW={HW} C={C}]", dx, R.gap_bwd(dp, HW), 2 * U24 * R.gap_bwd(dp.abs(), HW))


@pytest.mark.parametrize("C,Cp", [(3, 8), (3, 16), (8, 8), (5, 8)])
def test_nchw_to_nhwc_pads_with_exact_zeros(gpu, lib, C, Cp):
    B, H, W = 2, 5, 7
    x = randn((B, C, H, W), 1)
    out = torch.full((B, H, W, Cp), 3.0, device=gpu, dtype=BF16)
    ok(lib.ia_nchw_to_nhwc_bf16(PG(x), P(out), B, C, H, W, Cp, st()), "ia_nchw_to_nhwc_bf16")
    bits(f"nchw_to_nhwc[{C}->{Cp}]", out, R.nchw_to_nhwc(x, Cp))
    assert (out.cpu()[..., C:].view(torch.int16) == 0).all()


@pytest.mark.parametrize("in_padded,out_padded", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pad_rows_copies_between_layouts(gpu, lib, in_padded, out_padded):
    B, H, W, C = 2, 3, 5, 16
    x = randn((B, H + 2 * in_padded, W + 2 * in_padded, C), 1, 1.0, BF16)          # a padded input's border is ignored: leave it non-zero
    y = torch.full((B, H + 2 * out_padded, W + 2 * out_padded, C), 3.0, device=gpu, dtype=BF16)
    ok(lib.ia_pad_rows(PG(x), P(y), B, H, W, C, in_padded, out_padded, st()), "ia_pad_rows")
    bits(f"pad_rows[{in_padded}->{out_padded}]", y, R.pad_rows(x, in_padded, out_padded))


@pytest.mark.parametrize("Cout,Cg,kk,Cgp,ldw", [(5, 3, 49, 3, 152), (16, 64, 9, 64, 576), (4, 3, 9, 8, 72), (3, 8, 1, 8, 24)])
def test_conv_weight_pack_and_unpack(gpu, lib, Cout, Cg, kk, Cgp, ldw):
    w = randn((Cout, Cg, kk), 1)
    what = torch.full((Cout, ldw), 3.0, device=gpu, dtype=BF16)
    ok(lib.ia_conv_weight_pack(PG(w), P(what), Cout, Cg, kk, Cgp, ldw, st()), "ia_conv_weight_pack")
    bits("conv_weight_pack", what, R.weight_pack(w, Cgp, ldw))
    dwhat = randn((Cout, ldw), 2)
    dw0 = randn((Cout, Cg, kk), 3)
    dw = dw0.to(gpu)
    ok(lib.ia_conv_weight_unpack_grad(PG(dwhat), P(dw), Cout, Cg, kk, Cgp, ldw, st()), "ia_conv_weight_unpack_grad")
    bits("conv_weight_unpack_grad", dw, dw0 + R.weight_unpack_grad(dwhat, Cg, kk, Cgp).to(F32))       # one fp32 addition: correctly rounded


def _silu_inputs():
    x = torch.cat((torch.linspace(-20, 20, 1001), torch.tensor([0.0, -0.0, 88.0, -88.0, 1.278, -1.278, 2.0 ** -20])))
    x = torch.cat((x, torch.zeros(-x.numel() % 8))).to(BF16)
    return x, randn(x.shape, 1, 1.0, BF16), randn(x.shape, 2, 1.0, BF16), randn(x.shape, 3, 1.0, BF16)


def test_silu_fwd_against_fp64(gpu, lib):
    """silu(x) * scale over [-20, 20], 0 and +-88 (where __expf(-x) is near the end of the fp32 range).  The sigmoid's exponential
    is good to (2 |x| + 3) * 2^-24 (the constant log2 e and its product with x each put 2^-24 |x log2 e| into the exponent), then an
    addition, a quotient and the scale."""
    x, _, _, _ = _silu_inputs()
    scale = 1.7
    y = torch.empty(x.shape, device=gpu, dtype=BF16)
    ok(lib.ia_silu_fwd(PG(x), P(y), x.numel(), scale, st()), "ia_silu_fwd")
    want = R.silu(x, np.float32(scale).item())
    # exponential 2 |x| + 3, the addition 1, the quotient (2.5 ulp = 5 if it is the fast one), the scale 1
    bf16_close("silu_fwd", y, want, U24 * (2 * x.to(F64).abs() + 10) * want.abs() + TINY)


@pytest.mark.parametrize("use2,useadd", [(False, False), (False, True), (True, False), (True, True)])
def test_silu_bwd_and_bwd_sum_against_fp64(gpu, lib, use2, useadd):
    """dx = (dy [+ dy2]) * scale * s (1 + x (1 - s)) [+ dadd], s = sigmoid(x): ia_silu_bwd without dy2, ia_silu_bwd_sum with it, dadd
    NULL and not.  The bracket cancels near x = -1.278, so the fp32 term is taken on |gy scale s| (1 + |x| (1 - s))."""
    x, dy, dy2, dadd = _silu_inputs()
    scale = 1.7
    dx = torch.empty(x.shape, device=gpu, dtype=BF16)
    if use2:
        ok(lib.ia_silu_bwd_sum(PG(dy), PG(dy2), PG(x), PG(dadd) if useadd else None, P(dx), x.numel(), scale, st()), "ia_silu_bwd_sum")
    else:
        ok(lib.ia_silu_bwd(PG(dy), PG(x), PG(dadd) if useadd else None, P(dx), x.numel(), scale, st()), "ia_silu_bwd")
    sc = np.float32(scale).item()
    want = R.silu_bwd(dy, x, sc, dy2 if use2 else None, dadd if useadd else None)
    x64 = x.to(F64)
    sg = torch.sigmoid(x64)
    gy = dy.to(F64).abs() + (dy2.to(F64).abs() if use2 else 0.0)
    T = gy * sc * sg * (1.0 + x64.abs() * (1.0 - sg))
    # s is good to (2 |x| + 9) * 2^-24 (exponential 2 |x| + 3, addition, quotient 5) and enters twice; the sum of the gradients, four
    # products and the bracket's two operations: 8; then the addition of dadd
    a = U24 * ((4 * x64.abs() + 26) * T + (dadd.to(F64).abs() if useadd else 0.0) + want.abs()) + TINY
    bf16_close(f"silu_bwd[dy2 {use2}, dadd {useadd}]", dx, want, a)


# =============================================================================================================== LayerNorm backward
def _ln_chain(M):
    nb = min(512, (M + 3) // 4)
    rows = (M + nb * 4 - 1) // (nb * 4)
    # a wave's rows, 3 additions across the waves, the second stage: up to ceil(nb / 128) per partial chain, 2 to join the four
    # chains, 32 across the slices, the accumulation; 4 operations inside a term
    return rows + 3 + (nb + 127) // 128 + 2 + 32 + 1 + 4


@pytest.mark.parametrize("M,H", [(37, 768), (37, 1024), (2051, 768)])
def test_ln_bwd2_against_fp64_and_row_filter(gpu, lib, M, H):
    """ia_ln_bwd2 / ia_ln_bwd2_rows directly (the layer driver's test only asks for a cosine): dz, dgamma, dbeta, dbias against the fp64
    LayerNorm backward of dy + dy2 (+ dres); dz aliasing dy2; a row filter with dead rows whose inputs are zero gives the same bits as
    the unfiltered call and exact zeros in the dead rows.  M is no multiple of the 4 rows of a block.
    The kernel rounds dy + dy2 to bf16 before the LayerNorm backward (its comment says "summed in fp32"; the sum is, its result is
    not kept).  That rounding, up to 2^-8 |dy + dy2| gamma rstd, is part of the kernel's documented arithmetic on the training path
    and is left alone here; the gradients are drawn from a grid on which the sum is a bf16 number, so the fp64 reference of dy + dy2
    and the bars above apply unchanged."""
    z, dy, dres = randn((M, H), 1, 2.0, BF16), randn((M, H), 2, 1.0, BF16), randn((M, H), 4, 1.0, BF16)
    # dy2 on a grid that makes dy + dy2 a bf16 number whenever dy is: the kernel keeps the sum of the two upstream gradients in bf16
    dy = (dy.to(F32) * 4).round().div(4).clamp(-3, 3).to(BF16)
    dy2 = (randn((M, H), 3) * 4).round().div(4).clamp(-3, 3).to(BF16)
    gamma = torch.rand(H, generator=gen(5)) + 0.5
    zf = z.to(F64)
    mean = zf.mean(1).to(F32)
    rstd = (1.0 / torch.sqrt(zf.var(1, unbiased=False) + 1e-5)).to(F32)
    live = torch.rand(M, generator=gen(6)) < 0.6
    live[0], live[M - 1] = True, False
    ws_bytes = lib.ia_ln_bwd_workspace_bytes(M, H)
    ws = torch.empty(ws_bytes, device=gpu, dtype=torch.uint8)
    dv = lambda t: None if t is None else t.to(gpu)
    zd, md, rd, gd = dv(z), dv(mean), dv(rstd), dv(gamma)
    init = 0.5

    def run(dy_, dy2_, dres_, rows=None, alias=False):
        dyd, dy2d, dresd = dv(dy_), dv(dy2_), dv(dres_)
        dz = dy2d if alias else torch.full((M, H), 9.0, device=gpu, dtype=BF16)
        outs = [torch.full((H,), init, device=gpu) for _ in range(3)]
        if rows is None:
            ok(lib.ia_ln_bwd2(P(dyd), P(dy2d), P(dresd), P(zd), P(md), P(rd), P(gd), P(dz), None, *(P(o) for o in outs), M, H, 0.0, 0, 0, P(ws), ws_bytes,
                              1, st()), "ia_ln_bwd2")
        else:
            ok(lib.ia_ln_bwd2_rows(P(dyd), P(dy2d), P(dresd), P(zd), P(md), P(rd), P(gd), P(dz), None, *(P(o) for o in outs), M, H, 0.0, 0, 0,
                                   PG(rows), P(ws), ws_bytes, 1, st()), "ia_ln_bwd2_rows")
        return [dz.clone()] + outs

    tag = f"ln_bwd2[{M}x{H}]"
    c_row = nv_of(H) * 8 + 6 + 10
    gam = gamma.to(F64)
    xh = (zf - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]
    for name, d2 in (("dy2 NULL", None), ("dy + dy2", dy2)):
        got = run(dy, d2, dres)
        dsum = dy.to(F64) + (d2.to(F64) if d2 is not None else 0.0)
        assert torch.equal(R.bf16_round(dsum), dsum)
        dz64, dgamma64, dbeta64 = R.layernorm_bwd(dsum, z, mean, rstd, gamma)
        ga = (dsum * gam).abs()
        S_row = rstd.to(F64)[:, None] * (ga + ga.mean(1, keepdim=True) + xh.abs() * (ga * xh.abs()).mean(1, keepdim=True))
        bf16_close(f"{tag} dz ({name})", got[0], dz64 + dres.to(F64), (c_row + 1) * U24 * (S_row + dres.to(F64).abs()))
        c = _ln_chain(M)
        sum_close(f"{tag} dgamma ({name})", got[1], dgamma64 + init, (dsum * xh).abs().sum(0) + init, c)
        sum_close(f"{tag} dbeta ({name})", got[2], dbeta64 + init, dsum.abs().sum(0) + init, c)
        # dbias = column sums of the fp32 dz (before its rounding): the row's error scale, summed
        sum_close(f"{tag} dbias ({name})", got[3], (dz64 + dres.to(F64)).sum(0) + init, (S_row + dres.to(F64).abs()).sum(0) + init, c + c_row)
    plain = run(dy, dy2, dres)
    aliased = run(dy, dy2, dres, alias=True)
    for a, b, n in zip(aliased, plain, ("dz", "dgamma", "dbeta", "dbias")):
        bits(f"{tag} {n} with dz aliasing dy2", a, b)
    lv = live[:, None]
    dyz, dy2z, dresz = (torch.where(lv, t, torch.zeros((), dtype=BF16)) for t in (dy, dy2, dres))
    unfiltered = run(dyz, dy2z, dresz)
    filtered = run(dyz, dy2z, dresz, rows=live.to(torch.uint8))
    for a, b, n in zip(filtered, unfiltered, ("dz", "dgamma", "dbeta", "dbias")):
        bits(f"{tag} {n} under the row filter", a, b)
    assert (filtered[0].cpu()[~live].view(torch.int16) == 0).all(), "dead rows must be exact zeros"


# =============================================================================================================== arena / optimiser helpers
def test_transpose_bf16_batched_odd_sizes(gpu, lib):
    """The table is built the way arena.py builds it: {offset_lo, offset_hi, rows, cols} in uint32, max_tiles = the largest tile count.
    Sizes that are no multiple of the 64 x 64 tile or of the 2-element lanes; the gaps between the matrices keep their contents."""
    shapes = [(70, 130), (64, 64), (1, 200), (33, 7), (129, 1)]
    ent, off = [], 3
    for r, c in shapes:
        ent.append((off & 0xFFFFFFFF, off >> 32, r, c))
        off += r * c + 5
    src = randn((off,), 1, 1.0, BF16)
    dst = torch.full((off,), 3.0, device=gpu, dtype=BF16)
    table = torch.from_numpy(np.asarray(ent, dtype=np.uint32).reshape(-1, 4)).to(gpu)
    tiles = max(((r + 63) // 64) * ((c + 63) // 64) for _, _, r, c in ent)
    ok(lib.ia_transpose_bf16_batched(PG(src), P(dst), P(table), len(ent), tiles, st()), "ia_transpose_bf16_batched")
    want = torch.full((off,), 3.0, dtype=BF16)
    for o, _, r, c in ent:
        want[o:o + r * c] = src[o:o + r * c].view(r, c).t().reshape(-1)
    bits("transpose_bf16_batched", dst, want)


@pytest.mark.parametrize("n", [1, 3, 5, 1027, 2100001])
def test_casts_are_bit_exact(gpu, lib, n):
    x = randn((n,), 1)
    sp = torch.tensor([0.0, -0.0, 1e-40, 65504.0, 3.4e38, -3.4e38, float("inf"), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])[:n]
    x[:sp.numel()] = sp
    out = torch.full((n + 3,), 3.0, device=gpu, dtype=BF16)
    ok(lib.ia_cast_f32_to_bf16(PG(x), P(out), n, st()), "ia_cast_f32_to_bf16")
    bits("cast_f32_to_bf16", out[:n], x.to(BF16))
    assert (out[n:] == 3.0).all()
    back = torch.full((n + 3,), 3.0, device=gpu)
    ok(lib.ia_cast_bf16_to_f32(P(out), P(back), n, st()), "ia_cast_bf16_to_f32")
    bits("cast_bf16_to_f32", back[:n], x.to(BF16).to(F32))
    assert (back[n:] == 3.0).all()
