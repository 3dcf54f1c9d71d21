"""The CPU model of the GPU JPEG decoder (tests/jpeg_reference.py) against Pillow, the piece scheme against the sequential decode,
the host parser (item_alignment_amd/data/jpeg.py) against the model, the fall-back to Pillow and the row-dropping helper.  No GPU."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_reference as R


def _mismatches(**kw):
    bad = []
    for i, (name, buf) in enumerate(R.all_files()):
        if name.endswith("rst3"):
            continue
        hdr, coefs, status = R.reference_of(i)
        if status != 0 or not np.array_equal(R.reconstruct(hdr, coefs, **kw), R.pillow_rgb(buf)):
            bad.append(name)
    return bad


def test_reference_equals_pillow_in_every_byte():
    """480 small files (10 sizes x 4 samplings x 4 qualities x {plain, optimize, restart every block}) and 96 x 128 files of
    q95 4:4:4 and q75 4:2:0"""
    assert len(R.all_files()) == 483
    assert _mismatches() == []


def test_injected_faults_are_seen():
    """replication instead of the fancy upsampling, and a descale rounding constant off by one, each break the comparison"""
    assert _mismatches(fancy=False)
    assert _mismatches(descale_bias=1)
    assert _mismatches(descale_bias=-1)


@pytest.mark.parametrize("bits", [64, 128, 1024])
def test_piece_model_equals_sequential_decode(bits):
    files = R.all_files()
    for i in range(480, 483):
        hdr, coefs, status = R.reference_of(i)
        got, st, rounds = R.piece_coefficients(hdr, bits)
        assert st == 0 and status == 0
        for a, b in zip(got, coefs):
            assert np.array_equal(a, b), (files[i][0], bits)
        if bits == 128:
            # the streams resynchronise after a few hundred to a few thousand bits: more than one round, far fewer than the piece count
            assert rounds > 1, (files[i][0], rounds)


def test_piece_model_on_small_files():
    """every 7th file of the matrix (all samplings, restart segments of one block included) at the shortest piece"""
    for i in range(0, 480, 7):
        hdr, coefs, _ = R.reference_of(i)
        got, st, _ = R.piece_coefficients(hdr, 64)
        assert st == 0 and all(np.array_equal(a, b) for a, b in zip(got, coefs)), R.all_files()[i][0]


def test_host_parser_agrees_with_the_model():
    from item_alignment_amd.data.jpeg import parse_jpeg
    for i, (name, buf) in enumerate(R.all_files()):
        hdr = R.parse(buf)
        p = parse_jpeg(buf)
        assert p is not None and (p.width, p.height, p.ncomp) == (hdr["W"], hdr["H"], len(hdr["comps"])), name
        assert (p.hs, p.vs, p.mx, p.my) == (hdr["hmax"], hdr["vmax"], hdr["mx"], hdr["my"]) and p.ri == (hdr["dri"] or hdr["mx"] * hdr["my"])
        segs = R.segments(hdr["scan"])
        assert len(segs) == len(p.seg_len) and all(o % 4 == 0 for o in p.seg_off)
        for s, o, n in zip(segs, p.seg_off, p.seg_len):
            assert p.scan[o:o + n].tobytes() == s, name
        for c, comp in enumerate(hdr["comps"]):
            q = np.zeros(64, dtype=np.int64)
            q[R.ZIGZAG] = comp["q"]
            assert np.array_equal(q, p.qt[c])
            for t, table in ((2 * c, comp["dc"]), (2 * c + 1, comp["ac"])):      # the 9-bit look-ahead against the 16-bit table
                look = p.tables[t, :1024].view(np.uint16).astype(np.int64)
                full = R.lut16(table)[::128]
                short = (full >> 8) <= 9
                assert np.array_equal(np.where(short, full, 0), look), name


def _unsupported_files():
    from PIL import Image
    frame = R.photo(40, 30, 3)
    out = {}
    bio = io.BytesIO()
    Image.fromarray(frame).save(bio, "JPEG", quality=80, progressive=True)
    out["progressive"] = bio.getvalue()
    bio = io.BytesIO()
    Image.fromarray(frame).convert("CMYK").save(bio, "JPEG", quality=80)
    out["cmyk"] = bio.getvalue()
    bio = io.BytesIO()
    Image.fromarray(frame).save(bio, "PNG")
    out["png"] = bio.getvalue()
    good = R.encode(frame, 80, "4:2:0")
    out["cut-in-headers"] = good[:good.index(b"\xff\xc0") + 7]
    return out, good


def test_unsupported_files_fall_back_to_pillow(tmp_path):
    from item_alignment_amd.data.datasets import RawImage, load_image
    from item_alignment_amd.data.jpeg import JpegImage, parse_jpeg
    from item_alignment_amd.data.transforms import ImageTransform
    files, good = _unsupported_files()
    for name, buf in files.items():
        assert parse_jpeg(buf) is None and R.parse(buf) is None, name
    assert parse_jpeg(good) is not None
    # fill bytes inside the scan, a second SOS, 16-bit tables, an Adobe segment with transform 0, R G B ids without JFIF
    sos = good.index(b"\xff\xda")
    scan = sos + 2 + ((good[sos + 2] << 8) | good[sos + 3])
    assert parse_jpeg(good[:scan + 20] + b"\xff\xff" + good[scan + 20:]) is None
    assert parse_jpeg(good[:-2] + good[sos:scan] + good[scan:]) is None
    adobe0 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert parse_jpeg(good[:2] + adobe0 + good[2:]) is None and R.parse(good[:2] + adobe0 + good[2:]) is None
    nojfif = bytearray(good[:2] + good[good.index(b"\xff\xdb"):])
    assert parse_jpeg(bytes(nojfif)) is not None                                  # ids 1 2 3: libjpeg assumes YCbCr
    sof = nojfif.index(b"\xff\xc0")
    sos2 = nojfif.index(b"\xff\xda")
    for c, ch in enumerate(b"RGB"):
        nojfif[sof + 10 + 3 * c] = ch
        nojfif[sos2 + 5 + 2 * c] = ch
    assert parse_jpeg(bytes(nojfif)) is None and R.parse(bytes(nojfif)) is None
    for name in ("progressive", "cmyk", "png"):
        path = os.path.join(tmp_path, name + ".jpg")
        open(path, "wb").write(files[name])
        a = load_image(path, ImageTransform(32, True, seed=5), jpeg=True)
        b = load_image(path, ImageTransform(32, True, seed=5), raw=True)
        assert isinstance(a, RawImage) and torch.equal(a.u8, b.u8) and a.params == b.params
    path = os.path.join(tmp_path, "cut.jpg")
    open(path, "wb").write(files["cut-in-headers"])
    errs = []
    for kw in (dict(jpeg=True), dict(raw=True)):
        with pytest.raises(Exception) as e:
            load_image(path, ImageTransform(32, False), **kw)
        errs.append(type(e.value))
    assert errs[0] is errs[1]
    path = os.path.join(tmp_path, "good.jpg")
    open(path, "wb").write(good)
    a = load_image(path, ImageTransform(32, True, seed=5), jpeg=True)
    b = load_image(path, ImageTransform(32, True, seed=5), raw=True)
    assert isinstance(a, JpegImage) and a.params == b.params and a.data.numpy().tobytes() == good
    assert (a.plan.width, a.plan.height) == (40, 30)


def test_jpeg_image_pickles_cheaply():
    import pickle

    from item_alignment_amd.data.jpeg import JpegImage, parse_jpeg
    from item_alignment_amd.data.transforms import ImageTransform
    buf = R.encode(R.photo(400, 300, 1), 90, "4:2:0")
    item = JpegImage(torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()), parse_jpeg(buf), ImageTransform(64, True, seed=1).draw(400, 300))
    blob = pickle.dumps(item)
    assert len(blob) < 2 * len(buf) + 16384 and len(blob) < 400 * 300 * 3 // 2
    back = pickle.loads(blob)
    assert back.params == item.params and np.array_equal(back.plan.scan, item.plan.scan) and torch.equal(back.data, item.data)


def test_drop_rows():
    from item_alignment_amd.data.datasets import RawImageBatch
    from item_alignment_amd.data.jpeg import drop_rows
    batch = (["a", "b", "c"], ["x", "y", "z"], RawImageBatch([1, 2, 3]), torch.arange(6).view(3, 2), None, RawImageBatch([4, 5, 6]), torch.tensor([7, 8, 9]))
    assert drop_rows(batch, [True, True, True]) is batch
    out = drop_rows(batch, [True, False, True])
    assert out[0] == ["a", "c"] and out[1] == ["x", "z"] and out[2].items == [1, 3] and out[5].items == [4, 6] and out[4] is None
    assert torch.equal(out[3], torch.tensor([[0, 1], [4, 5]])) and torch.equal(out[6], torch.tensor([7, 9]))
    out = drop_rows(batch, [False, False, False])
    assert out[0] == [] and len(out[2]) == 0 and out[3].shape == (0, 2)


def test_layout_is_bounded_and_aligned():
    """the chunking keeps the coefficient workspace under its bound, and every offset the kernels rely on is aligned"""
    from item_alignment_amd.data import jpeg as J
    plans = [J.parse_jpeg(buf) for _, buf in R.all_files()[470:483]]
    lay = J.GpuJpegDecoder.layout(plans, 128)
    d = lay["desc"]
    assert (d[:, J.D_COEF] % 8 == 0).all() and (d[:, J.D_PLANE] % 16 == 0).all() and (lay["seg_off"] % 4 == 0).all()
    assert lay["coef_elements"] == sum(p.coef_elements for p in plans) and lay["pieces"] == len(lay["piece_seg"])
    big = J.parse_jpeg(R.all_files()[480][1])
    n = J.COEF_CHUNK_BYTES // (big.coef_elements * 2)
    chunks = J.GpuJpegDecoder.chunks([big] * (2 * n + 1))
    assert [len(c) for c in chunks] == [n, n, 1]
    assert J.MAX_PIXELS * 6 + 64 * 64 * 2 <= J.COEF_CHUNK_BYTES
