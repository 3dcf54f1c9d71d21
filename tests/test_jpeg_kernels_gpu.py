"""The GPU JPEG decoder (csrc/jpeg.hip through item_alignment_amd/data/jpeg.py) against the CPU model (tests/jpeg_reference.py) and
against Pillow: each stage on its own, the whole batched decode, and damaged scans.  Equality everywhere, no tolerance."""
import numpy as np
import pytest
import torch

import jpeg_reference as R

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A      # what the coefficient buffer holds before a decode: the guards around every component grid must still hold it


def _plans(files):
    from item_alignment_amd.data.jpeg import parse_jpeg
    plans = [parse_jpeg(buf) for _, buf in files]
    assert all(p is not None for p in plans)
    return plans


def _expected_buffer(plans, lay, coefs_of):
    """the whole coefficient buffer as it must look after the entropy stage: the pattern, with every grid replaced"""
    from item_alignment_amd.data import jpeg as J
    want = np.full(lay["coef_elements"], PATTERN, dtype=np.int16)
    grid = np.zeros(lay["coef_elements"], dtype=bool)
    for i, p in enumerate(plans):
        o = int(lay["desc"][i, J.D_COEF])
        for c in range(p.ncomp):
            n = p.blocks[c] * 64
            if coefs_of is not None:
                ref = coefs_of(i)[c]
                assert ref.shape == p.grid(c) + (64,)
                want[o:o + n] = ref.reshape(-1)
            grid[o:o + n] = True
            o += n + J.GUARD
    return want, grid


@pytest.mark.parametrize("bits", [128, 1024])
def test_entropy_stage_equals_the_reference(gpu, bits):
    """483 files in one call: every coefficient of every MCU-padded grid, and every guard element between the grids"""
    from item_alignment_amd.data.jpeg import GpuJpegDecoder
    files = R.all_files()
    plans = _plans(files)
    dec = GpuJpegDecoder(gpu)
    coef, stat, lay, _, _ = dec.entropy(plans, bits, fill=PATTERN)
    want, grid = _expected_buffer(plans, lay, lambda i: R.reference_of(i)[1])
    assert not grid.all() and (~grid).sum() == sum((p.ncomp + 1) * 64 for p in plans)
    got = coef[:lay["coef_elements"]].cpu()
    stat = stat.cpu().numpy()
    assert (stat[0] == 0).all(), [files[i][0] for i in np.flatnonzero(stat[0])]
    if not torch.equal(got, torch.from_numpy(want)):
        bad = np.flatnonzero(got.numpy() != want)
        raise AssertionError(f"{len(bad)} elements differ, first at {bad[:8]}, guards touched: {int((~grid)[bad].sum())}")
    if bits == 128:
        for i in (480, 481, 482):                                         # pass-B rounds: as many as the model needs, more than one,
            rounds = R.piece_coefficients(R.reference_of(i)[0], bits)[2]     # far fewer than the pieces of the longest segment
            assert stat[1, i] == rounds and 1 < rounds < lay["desc"][i, 12], (files[i][0], stat[1, i], rounds)


def test_reconstruction_stage_equals_pillow(gpu):
    """from the REFERENCE's coefficients: 7 sizes (chroma planes 1, 2 and 3 samples wide among them) x 4 samplings x q5 (saturation) / q100"""
    from item_alignment_amd.data.jpeg import GpuJpegDecoder
    files = R.all_files()
    sizes = {"1x1", "7x4", "9x3", "40x6", "13x17", "33x31", "5x64"}
    pick = [i for i, (name, _) in enumerate(files[:480]) if name.split("-")[0] in sizes and name.split("-")[2] in ("q5", "q100") and name.endswith("v0")]
    assert len(pick) == 7 * 4 * 2
    pick += [480, 481]
    plans = _plans([files[i] for i in pick])
    dec = GpuJpegDecoder(gpu)
    lay = dec.layout(plans, 1024)
    want, _ = _expected_buffer(plans, lay, lambda j: R.reference_of(pick[j])[1])
    dev, ptrs, _ = dec._upload(lay)
    frames = dec.reconstruct(plans, torch.from_numpy(want).to(gpu), lay, ptrs)
    torch.cuda.synchronize()
    for j, i in enumerate(pick):
        assert np.array_equal(frames[j].cpu().numpy(), R.pillow_rgb(files[i][1])), files[i][0]


def _guards_intact(dec, plans, bits=1024):
    lay = dec.layout(plans, bits)
    _, grid = _expected_buffer(plans, lay, None)
    got = dec._coef[:lay["coef_elements"]].cpu().numpy()
    return bool((got[~grid] == PATTERN).all())


def test_whole_decode_in_one_batched_call(gpu):
    from item_alignment_amd.data.jpeg import GpuJpegDecoder
    batch = [("a", R.encode(R.photo(96, 128, 11), 95, "4:4:4")), ("b", R.encode(R.photo(131, 77, 12), 75, "4:2:0")),
             ("c", R.encode(R.photo(64, 200, 13), 85, "4:2:2")), ("d", R.encode(R.photo(50, 50, 14), 60, None, gray=True)),
             ("e", R.encode(R.photo(203, 99, 15), 80, "4:2:0", restart_marker_blocks=5)),
             ("f", R.encode(R.photo(75, 91, 16), 90, "4:2:2", optimize=True)), ("g", R.encode(R.photo(17, 9, 17), 30, "4:4:4"))]
    plans = _plans(batch)
    dec = GpuJpegDecoder(gpu)
    frames, status = dec.decode(plans, fill=PATTERN)
    assert (status == 0).all() and _guards_intact(dec, plans)
    together = [f.cpu().numpy() for f in frames]
    for (name, buf), p, got in zip(batch, plans, together):
        alone, st = dec.decode([p])
        assert st[0] == 0 and np.array_equal(alone[0].cpu().numpy(), got), name
        assert np.array_equal(got, R.pillow_rgb(buf)), name


def test_800x800_file_equals_pillow(gpu):
    from item_alignment_amd.data.jpeg import GpuJpegDecoder
    buf = R.encode(R.photo(800, 800, 21), 90, "4:2:0")
    dec = GpuJpegDecoder(gpu)
    frames, status = dec.decode(_plans([("big", buf)]))
    assert status[0] == 0 and 1 <= dec.last_rounds[0] < 64
    assert np.array_equal(frames[0].cpu().numpy(), R.pillow_rgb(buf))


def _damaged():
    good = R.all_files()[[n for n, _ in R.all_files()].index("33x31-4:2:0-q90-v0")][1]
    sos = good.index(b"\xff\xda")
    scan = sos + 2 + ((good[sos + 2] << 8) | good[sos + 3])
    n = len(good) - 2 - scan
    out = [("cut", good[:scan + (6 * n) // 10])]
    for at, bit in ((n // 2, 3), (n // 3, 0), (n - 4, 6)):
        b = bytearray(good)
        b[scan + at] ^= 1 << bit
        out.append((f"flip-{at}-{bit}", bytes(b)))
    return out


def test_malformed_scans_report_a_status_and_touch_nothing_else(gpu):
    """A scan cut at 60 % and scans with one flipped bit: the image either decodes completely or comes back with a non-zero status,
    exactly where the CPU model says so; the guards stay intact; the fall-back gives what Pillow gives or None where Pillow raises."""
    from item_alignment_amd.data.jpeg import GpuJpegDecoder, JpegImage, decode_with_fallback, parse_jpeg
    files = [(n, b) for n, b in _damaged() if parse_jpeg(b) is not None]
    assert len(files) >= 3 and files[0][0] == "cut"
    plans = _plans(files)
    dec = GpuJpegDecoder(gpu)
    frames, status = dec.decode(plans, fill=PATTERN)
    assert _guards_intact(dec, plans)
    assert status[0] != 0
    items = [JpegImage(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()), p, None) for (_, b), p in zip(files, plans)]
    fixed = decode_with_fallback(dec, items)
    for (name, buf), st, frame, fb in zip(files, status, frames, fixed):
        hdr = R.parse(buf)
        ref, ref_status = R.sequential_coefficients(hdr)
        assert (st != 0) == (ref_status != 0), name
        assert tuple(frame.shape) == (31, 33, 3)
        try:
            want = R.pillow_rgb(buf)
        except Exception:
            want = None
        if st != 0:
            assert (fb is None) == (want is None), name
            if want is not None:
                assert np.array_equal(fb.cpu().numpy(), want), name
        else:
            assert np.array_equal(frame.cpu().numpy(), R.reconstruct(hdr, ref)), name      # a complete decode of what the bits say
