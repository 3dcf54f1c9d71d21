"""The forward-only entry points of csrc/conv.hip through the C ABI against the fp64 reference of tests/conv_act_reference.py, element by
element: ia_conv3x3_padded_fwd_act and ia_conv3x3_s2_padded_fwd_act (the direct kernels whose epilogue stores
bf16(silu(acc + bias) * act_scale)), in both output layouts, and ia_silu_gap_fwd.

Operands as in tests/test_conv_kernels_gpu.py (whose buffers this file borrows): every input in the middle of a NaN-filled buffer with
a zero border, every output pre-filled -- here with the bit pattern 0x5A5A, which no computed element is likely to equal and which the
border of a bordered output (y_compact = 0: "the border belongs to the caller") and the guards around every output must still hold bit
for bit afterwards.  The bars are conv_act_reference.act_bar / gap_bar: derived, checked on the host against a CPU model and two
injected faults by tests/test_conv_act_reference_host.py.

Worst error / bar seen on one MI355X over all cases (recorded figures, no input to any bar; a correctly rounded bf16 store alone
reaches 1.0 of its 2^-8 allowance just above a power of two):
  ia_conv3x3_padded_fwd_act      0.984        ia_conv3x3_s2_padded_fwd_act   0.913        ia_silu_gap_fwd   0.099

The plain ia_conv3x3_padded_fwd shares its kernel template with the new variant: its output on fixed integer-derived operands is held
to SHA-256 digests recorded with the library built from the commit before the variant existed (tests/golden/conv_act/plain_fwd.json).
"""
import hashlib
import json
import os

import pytest
import torch

import conv_act_reference as A
import conv_reference as R
import test_conv_kernels_gpu as K

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
PATTERN = 0x5A5A
SCALES = (1.0, 0.6180339887)
IA_ERR_UNSUPPORTED = -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_act", "plain_fwd.json")
GOLDEN_SHAPES = [(2, 9, 31, 64, 64, 1), (2, 9, 31, 16, 32, 1), (1, 10, 33, 384, 384, 6)]
S2_ACT_MAPS = [(1, 1, 1), (2, 17, 61), (2, 15, 59)]
S2_ACT_SHAPES = [R.conv3(B, H, W, ci, co, g, 2) for ci, co, g in R.S2_CHANNELS for B, H, W in S2_ACT_MAPS]
GAP_SHAPES = [(1, 1, 8), (3, 7, 3072), (2, 625, 2304), (1, 169, 64)]
name = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def pool(gpu):
    return R.normal_pool(torch.Generator(device="cuda").manual_seed(4127))


def patterned(shape):
    """an output buffer whose every bf16 element, guards included, holds PATTERN"""
    b = K.Buf(shape, BF16, K.SENT, fill=K.SENT)
    K.bits(b.whole).fill_(PATTERN)
    b.before = b.whole.clone()
    return b


def check_act(entry, s, ops, got, scale, where):
    want, bar = A.act_reference(s, ops, scale), A.act_bar(s, ops, scale)
    g64 = got.to(F64)
    print("%-30s %-44s worst error / bar %.3f" % (entry, where, R.worst_ratio(g64, want, bar)))
    bad = R.first_bad_nd(g64, want, bar)
    assert bad is None, "%s %s: %s" % (entry, where, bad)


@pytest.mark.parametrize("s", R.DIRECT_SHAPES + R.DIRECT_GROUP_SHAPES + R.DIRECT_WALK_SHAPES[:1], ids=name)
def test_stride1_act_epilogue(lib, pool, s):
    """every pair of DCONV_PAIRS at the tile-edge maps, 64 -> 64 with 2 and 6 groups, and the 64-group walk (three tiles per workgroup);
    both layouts of y, act_scale 1 and not 1"""
    B, H, W, Cin, Cout, g = s.B, s.H, s.W, s.C, s.Cout, s.groups
    ops = R.normal_operands(pool, s, "cuda")
    xp, what, bias = K.inp(R.to_bordered(ops["x"])), K.inp(ops["what"]), K.inp(ops["bias"], F32)
    for yc in (0, 1):
        for scale in SCALES:
            where = name(s[:5] + (g,)) + (" compact" if yc else " bordered") + " scale %.3f" % scale
            y = patterned((B, H, W, Cout) if yc else (B, H + 2, W + 2, Cout))
            K.ok(lib.ia_conv3x3_padded_fwd_act(xp.ptr(), what.ptr(), bias.ptr(), y.ptr(), B, H, W, Cin, Cout, g, scale, yc, K.sp()), "fwd_act")
            torch.cuda.synchronize()
            (y.guards_unchanged if yc else y.border_unchanged)("fwd_act " + where + ": y")
            check_act("conv3x3_padded_fwd_act", s, ops, y.v if yc else R.interior(y.v), scale, where)
    for nm, b in (("xp", xp), ("what", what), ("bias", bias)):
        b.unchanged(name(s) + ": input " + nm)


@pytest.mark.parametrize("s", S2_ACT_SHAPES, ids=name)
def test_stride2_act_epilogue(lib, pool, s):
    """64 g -> 64 g with g = 1, 2, 6 and the shared-input 64 -> 128 / 192 forms at a 1 x 1 map, an odd map one past a tile and an odd map
    inside one; both layouts of y"""
    B, H, W, Cin, Cout, g = s.B, s.H, s.W, s.C, s.Cout, s.groups
    assert lib.ia_conv3x3_s2_supported(Cin, Cout, g) == 1
    Ho, Wo = R.out_hw(s)
    ops = R.normal_operands(pool, s, "cuda")
    xp, what, bias = K.inp(R.to_bordered(ops["x"])), K.inp(ops["what"]), K.inp(ops["bias"], F32)
    for yc in (0, 1):
        for scale in SCALES:
            where = name(s[:5] + (g,)) + (" compact" if yc else " bordered") + " scale %.3f" % scale
            y = patterned((B, Ho, Wo, Cout) if yc else (B, Ho + 2, Wo + 2, Cout))
            K.ok(lib.ia_conv3x3_s2_padded_fwd_act(xp.ptr(), what.ptr(), bias.ptr(), y.ptr(), B, H, W, Cin, Cout, g, scale, yc, K.sp()), "s2_fwd_act")
            torch.cuda.synchronize()
            (y.guards_unchanged if yc else y.border_unchanged)("s2_fwd_act " + where + ": y")
            check_act("conv3x3_s2_padded_fwd_act", s, ops, y.v if yc else R.interior(y.v), scale, where)
    for nm, b in (("xp", xp), ("what", what), ("bias", bias)):
        b.unchanged(name(s) + ": input " + nm)


@pytest.mark.parametrize("Cin,Cout,groups", [(256, 256, 1), (128, 64, 1), (65 * 64, 65 * 64, 65)])
def test_pairs_without_a_direct_kernel_are_refused(lib, Cin, Cout, groups):
    """no view-GEMM form of the epilogue exists: IA_ERR_UNSUPPORTED before any launch, the output still the pattern (the same shapes run
    through the plain ia_conv3x3_padded_fwd); the stride-2 entry point refuses what ia_conv3x3_s2_supported refuses"""
    B, H, W = 1, 5, 7
    x = K.Buf((B, H + 2, W + 2, Cin), BF16, K.NAN, fill=0.0)
    w = K.Buf((Cout, 9 * (Cin // groups)), BF16, K.NAN, fill=0.0)
    y = patterned((B, H + 2, W + 2, Cout))
    assert lib.ia_conv3x3_padded_fwd_act(x.ptr(), w.ptr(), None, y.ptr(), B, H, W, Cin, Cout, groups, 1.0, 0, K.sp()) == IA_ERR_UNSUPPORTED
    if not lib.ia_conv3x3_s2_supported(Cin, Cout, groups):
        assert lib.ia_conv3x3_s2_padded_fwd_act(x.ptr(), w.ptr(), None, y.ptr(), B, H, W, Cin, Cout, groups, 1.0, 0, K.sp()) == IA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    y.unchanged("refused call: y")


# ------------------------------------------------------------------------------------------------ the plain forward did not move
def golden_operands(shape):
    """integer-derived bf16 operands, the same on every device and library version: multiples of 1/64 in [-2, 2] from a multiplicative hash
    of the element index (x, bias) and multiples of 1/512 in [-1/4, 1/4] (what)"""
    B, H, W, Cin, Cout, g = shape
    def draw(n, mult, div):
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        return ((((i * mult + 12345) & 0xFFFFFFFF) >> 13) % 257 - 128).to(F32) / div
    x = draw(B * H * W * Cin, 2654435761, 64.0).view(B, H, W, Cin)
    what = draw(Cout * 9 * (Cin // g), 2246822519, 512.0).view(Cout, 9 * (Cin // g))
    bias = draw(Cout, 3266489917, 64.0)
    return x, what, bias


def plain_fwd_digest(fn, stream, shape):
    """SHA-256 of the whole bordered output buffer (pattern in the border) of ia_conv3x3_padded_fwd `fn` on golden_operands"""
    B, H, W, Cin, Cout, g = shape
    x, what, bias = golden_operands(shape)
    xp, wb, bb = K.inp(R.to_bordered(x)), K.inp(what), K.inp(bias, F32)
    y = patterned((B, H + 2, W + 2, Cout))
    rc = fn(xp.ptr(), wb.ptr(), bb.ptr(), y.ptr(), B, H, W, Cin, Cout, g, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return hashlib.sha256(K.bits(y.v).cpu().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=name)
def test_plain_forward_is_bit_identical_to_the_recorded_parent(lib, shape):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert plain_fwd_digest(lib.ia_conv3x3_padded_fwd, K.sp(), shape) == want[name(shape)]


# ------------------------------------------------------------------------------------------------ SiLU + global average pool
@pytest.mark.parametrize("B,HW,C", GAP_SHAPES)
def test_silu_gap(lib, B, HW, C):
    """one pixel; 3072 channels (more column threads than a block); 625 pixels (nine slices, the last one short) at l0's width; 169 pixels
    at 64 channels (row lanes folded through LDS)"""
    g = torch.Generator(device="cuda").manual_seed(77 + HW)
    x = A.gap_input(g, B, HW, C, "cuda")
    for scale in (1.0, 1.7):
        xb = K.inp(x)
        wsb = lib.ia_gap_workspace_bytes(B, HW, C)
        ws = K.workspace(wsb)
        out = K.Buf((B, C), F32, K.SENT, fill=K.NAN)
        K.ok(lib.ia_silu_gap_fwd(xb.ptr(), out.ptr(), B, HW, C, scale, ws.data_ptr(), wsb, K.sp()), "silu_gap")
        torch.cuda.synchronize()
        K.ws_tail_ok(ws, wsb, "silu_gap")
        out.guards_unchanged("silu_gap: pooled")
        xb.unchanged("silu_gap: x")
        want, bar = A.gap_reference(x, scale), A.gap_bar(x, scale)
        got = out.v.to(F64)
        print("silu_gap_fwd %dx%dx%d scale %.1f worst error / bar %.3f" % (B, HW, C, scale, R.worst_ratio(got, want, bar)))
        bad = R.first_bad_nd(got, want, bar)
        assert bad is None, bad
    assert lib.ia_silu_gap_fwd(xb.ptr(), out.ptr(), B, HW, C, 1.0, ws.data_ptr(), wsb - 1 if wsb > 1 else 0, K.sp()) == K.IA_ERR_WORKSPACE
