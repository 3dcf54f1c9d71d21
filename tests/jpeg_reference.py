"""CPU model of the GPU JPEG decoder (item_alignment_amd/data/jpeg.py + csrc/jpeg.hip), in plain Python / numpy.

Nothing here imports the package: the header walk, the Huffman tables, the step function, the piece scheme and the back end are
written a second time, the slow and obvious way, so that a test comparing the two compares two derivations.

  parse(buf)                          headers -> dict (or None for what the decoder does not support)
  sequential_coefficients(hdr)        one walk over each restart segment -> per component int16 [bh, bw, 64] (natural order, DC summed)
  piece_coefficients(hdr, bits)       the same coefficients through the piece scheme: pass A, the pass-B rounds, the scan, pass C;
                                      also returns the largest number of pass-B rounds any segment needed and the status
  reconstruct(hdr, coefs)             dequantisation, accurate integer IDCT, fancy upsampling, YCbCr -> RGB: uint8 [H, W, 3]
  decode_rgb(buf)                     parse + sequential_coefficients + reconstruct
The two keyword switches of reconstruct (`fancy`, `descale_bias`) exist so that a test can break the arithmetic on purpose.
"""
import re

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
NO_LENGTH = {0x01, 0xD8} | set(range(0xD0, 0xD8))


def parse(buf):
    """Walk the segments by their lengths.  Returns None for everything outside the supported class (ISSUE / DESIGN §4.7)."""
    b = bytes(buf)
    if len(b) < 4 or b[0:2] != b"\xff\xd8":
        return None
    qt, huff, sof, dri, jfif, adobe = {}, {}, None, 0, False, None
    pos = 2
    try:
        while True:
            if b[pos] != 0xFF:
                return None
            m = b[pos + 1]
            if m == 0xFF:
                pos += 1
                continue
            if m in NO_LENGTH:
                pos += 2
                continue
            n = (b[pos + 2] << 8) | b[pos + 3]
            seg = b[pos + 4:pos + 2 + n]
            if len(seg) != n - 2:
                return None
            if m == 0xDB:
                i = 0
                while i < len(seg):
                    if seg[i] >> 4:
                        return None                                    # 16-bit table
                    qt[seg[i] & 15] = np.frombuffer(seg[i + 1:i + 65], dtype=np.uint8).astype(np.int32)
                    i += 65
            elif m == 0xC4:
                i = 0
                while i < len(seg):
                    counts = list(seg[i + 1:i + 17])
                    nv = sum(counts)
                    huff[(seg[i] >> 4, seg[i] & 15)] = (counts, list(seg[i + 17:i + 17 + nv]))
                    i += 17 + nv
            elif m in (0xC0, 0xC1):
                if sof is not None:
                    return None
                sof = dict(P=seg[0], H=(seg[1] << 8) | seg[2], W=(seg[3] << 8) | seg[4],
                           comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
            elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
                return None                                            # progressive, lossless, arithmetic, hierarchical
            elif m == 0xDD:
                dri = (seg[0] << 8) | seg[1]
            elif m == 0xE0 and seg[:5] == b"JFIF\0":
                jfif = True
            elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
            elif m == 0xDC:
                return None                                            # DNL
            elif m == 0xDA:
                break
            elif m == 0xD9:
                return None
            pos += 2 + n
        if sof is None or sof["P"] != 8 or sof["H"] == 0 or sof["W"] == 0 or len(sof["comps"]) not in (1, 3):
            return None
        nc = len(sof["comps"])
        if seg[0] != nc or tuple(seg[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
            return None
        sel = {seg[1 + 2 * c]: (seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(nc)}
        comps = []
        for cid, h, v, tq in sof["comps"]:
            if cid not in sel or tq not in qt or (0, sel[cid][0]) not in huff or (1, sel[cid][1]) not in huff:
                return None
            comps.append(dict(h=h, v=v, q=qt[tq], dc=huff[(0, sel[cid][0])], ac=huff[(1, sel[cid][1])]))
        if [seg[1 + 2 * c] for c in range(nc)] != [c[0] for c in sof["comps"]]:
            return None
        if nc == 1:
            comps[0]["h"] = comps[0]["v"] = 1
        else:
            ids = [c[0] for c in sof["comps"]]
            if adobe is not None:
                if adobe != 1:
                    return None
            elif not jfif and ids != [1, 2, 3]:
                return None                                            # libjpeg would guess RGB (or an unknown id set) here
            if (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
                return None
        start = pos + 2 + n
    except IndexError:
        return None
    m = re.search(rb"\xff[^\x00\xd0-\xd7]", b[start:])
    end = start + m.start() if m else len(b)
    if m and b[start + m.start() + 1] == 0xFF:
        return None                                                    # fill bytes inside the scan
    if m is None:
        pass                                                           # a file cut inside its scan: decode what is there
    elif b[start + m.start() + 1] != 0xD9:
        return None                                                    # another scan, DNL, ...
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    W, H = sof["W"], sof["H"]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    for c in comps:
        c["bw"], c["bh"] = mx * c["h"], my * c["v"]
        c["pw"], c["ph"] = -(-W * c["h"] // hmax), -(-H * c["v"] // vmax)
    return dict(W=W, H=H, comps=comps, hmax=hmax, vmax=vmax, mx=mx, my=my, dri=dri, scan=b[start:end])


def segments(scan):
    """restart segments of the scan, unstuffed: byte by byte"""
    out, cur, i = [], bytearray(), 0
    while i < len(scan):
        c = scan[i]
        if c == 0xFF and i + 1 < len(scan):
            n = scan[i + 1]
            if n == 0:
                cur.append(0xFF)
                i += 2
                continue
            if 0xD0 <= n <= 0xD7:
                out.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
        cur.append(c)
        i += 1
    out.append(bytes(cur))
    return out


def lut16(table):
    """canonical Huffman codes -> 65536-entry table of (length << 8 | symbol); 0 = no code matches these 16 bits"""
    counts, vals = table
    lut = np.zeros(65536, dtype=np.int32)
    code, i = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >> length:
                return lut                                             # over-subscribed table: the rest matches nothing
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[i]
            code += 1
            i += 1
        code <<= 1
    return lut


def extend(v, t):
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


class Segment:
    """One restart segment as a bit string; bits beyond its end read as 1."""

    def __init__(self, data, hdr):
        self.nbits = 8 * len(data)
        self.pad = 64
        self.big = int.from_bytes(data + b"\xff" * (self.pad // 8), "big")
        self.total = self.nbits + self.pad
        self.blk_comp = [ci for ci, c in enumerate(hdr["comps"]) for _ in range(c["h"] * c["v"])]
        self.dc = [lut16(c["dc"]) for c in hdr["comps"]]
        self.ac = [lut16(c["ac"]) for c in hdr["comps"]]

    def peek(self, p, n):
        if n == 0:
            return 0
        if p + n > self.total:                                         # only ever far beyond the end
            return (1 << n) - 1
        return (self.big >> (self.total - p - n)) & ((1 << n) - 1)

    def step(self, p, blk, k):
        """One symbol.  Returns (p', blk', k', ended a block, k of the coefficient or -1, value, error).  A code that matches
        nothing reads as 16 bits of symbol 0 (DC category 0 / end of block) and is an error."""
        c = self.blk_comp[blk]
        e = int((self.dc if k == 0 else self.ac)[c][self.peek(p, 16)])
        err = e == 0
        length, sym = (16, 0) if err else (e >> 8, e & 255)
        p += length
        at, val = -1, 0
        if k == 0:
            t = sym & 15
            at, val = 0, extend(self.peek(p, t), t)
            p += t
            k = 1
        else:
            r, s = sym >> 4, sym & 15
            if s == 0:
                k = k + 16 if r == 15 else 64
            else:
                k += r
                if k > 63:
                    err = True
                else:
                    at, val = k, extend(self.peek(p, s), s)
                p += s
                k += 1
        done = k >= 64
        if done:
            k, blk = 0, (blk + 1) % len(self.blk_comp)
        return p, blk, k, done, at, val, err


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _block_slot(hdr, g):
    """global block number in scan order -> (component, block row, block column) of the MCU-padded grids"""
    comps = hdr["comps"]
    bpm = sum(c["h"] * c["v"] for c in comps)
    mcu, b = divmod(g, bpm)
    for ci, c in enumerate(comps):
        n = c["h"] * c["v"]
        if b < n:
            return ci, (mcu // hdr["mx"]) * c["v"] + b // c["h"], (mcu % hdr["mx"]) * c["h"] + b % c["h"]
        b -= n
    raise AssertionError


def _segment_plan(hdr):
    comps = hdr["comps"]
    bpm = sum(c["h"] * c["v"] for c in comps)
    mcus = hdr["mx"] * hdr["my"]
    ri = hdr["dri"] or mcus
    segs = segments(hdr["scan"])
    nseg = -(-mcus // ri)
    return bpm, mcus, ri, segs, nseg


def _empty(hdr):
    return [np.zeros((c["bh"], c["bw"], 64), dtype=np.int16) for c in hdr["comps"]]


def sequential_coefficients(hdr):
    """-> (coefficients, status)"""
    bpm, mcus, ri, segs, nseg = _segment_plan(hdr)
    out, status = _empty(hdr), 0
    for si in range(nseg):
        expected = min(ri, mcus - si * ri) * bpm
        if si >= len(segs):
            status = 1
            continue
        seg = Segment(segs[si], hdr)
        p = blk = k = nb = 0
        pred = [0] * len(hdr["comps"])
        while nb < expected and p < seg.nbits:
            ci, row, col = _block_slot(hdr, si * ri * bpm + nb)
            p, blk, k, done, at, val, err = seg.step(p, blk, k)
            status |= int(err)
            if at == 0:
                pred[ci] += val
                out[ci][row, col, 0] = _wrap16(pred[ci])
            elif at > 0:
                out[ci][row, col, ZIGZAG[at]] = _wrap16(val)
            nb += done
        if nb < expected:
            status = 1
    return out, status


def piece_coefficients(hdr, subseq_bits):
    """-> (coefficients, status, most pass-B rounds in which a piece of one segment still changed)"""
    assert subseq_bits % 32 == 0 and subseq_bits >= 64
    bpm, mcus, ri, segs, nseg = _segment_plan(hdr)
    nc = len(hdr["comps"])
    out, status, max_rounds = _empty(hdr), 0, 0
    for si in range(nseg):
        expected = min(ri, mcus - si * ri) * bpm
        if si >= len(segs):
            status = 1
            continue
        seg = Segment(segs[si], hdr)
        npieces = max(1, -(-seg.nbits // subseq_bits))

        def run(i, entry):
            p, blk, k = entry
            end = min((i + 1) * subseq_bits, seg.nbits)
            n, dcs = 0, [0] * nc
            while p < end:
                ci = seg.blk_comp[blk]
                p, blk, k, done, at, val, _ = seg.step(p, blk, k)
                if at == 0:
                    dcs[ci] += val
                n += done
            return (p, blk, k), n, dcs

        # pass A
        entry = [(i * subseq_bits, 0, 0) for i in range(npieces)]
        res = [run(i, entry[i]) for i in range(npieces)]
        # pass B: bounded by the piece count, ends early when nothing changed
        rounds = 0
        for _ in range(npieces):
            prev_exit = [r[0] for r in res]
            changed = False
            for i in range(1, npieces):
                if prev_exit[i - 1] != entry[i]:
                    entry[i] = prev_exit[i - 1]
                    res[i] = run(i, entry[i])
                    changed = True
            if not changed:
                break
            rounds += 1
        max_rounds = max(max_rounds, rounds)
        # scan + pass C
        first, pred0 = 0, [0] * nc
        for i in range(npieces):
            p, blk, k = entry[i]
            end = min((i + 1) * subseq_bits, seg.nbits)
            nb, pred = first, list(pred0)
            while p < end and nb < expected:
                ci, row, col = _block_slot(hdr, si * ri * bpm + nb)
                p, blk, k, done, at, val, err = seg.step(p, blk, k)
                status |= int(err)
                if at == 0:
                    pred[ci] += val
                    out[ci][row, col, 0] = _wrap16(pred[ci])
                elif at > 0:
                    out[ci][row, col, ZIGZAG[at]] = _wrap16(val)
                nb += done
            first += res[i][1]
            pred0 = [a + b for a, b in zip(pred0, res[i][2])]
        if first < expected:
            status = 1
    return out, status, max_rounds


# ---------------------------------------------------------------------------------------------------------------- back end
F0_298, F0_390, F0_541, F0_765, F0_899, F1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F1_501, F1_847, F1_961, F2_053, F2_562, F3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _idct_1d(i, n, bias=0):
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * F0_541
    t2 = z1 - i6 * F1_847
    t3 = z1 + i2 * F0_765
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F1_175
    a0, a1, a2, a3 = a0 * F0_298, a1 * F2_053, a2 * F3_072, a3 * F1_501
    z1, z2 = z1 * -F0_899, z2 * -F2_562
    z3, z4 = z3 * -F1_961 + z5, z4 * -F0_390 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    outs = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    return [(v + (1 << (n - 1)) + bias) >> n for v in outs]


def idct_plane(coefs, q, descale_bias=0):
    """coefs int16 [bh, bw, 64] natural order, q [64] in zigzag order -> uint8 plane [bh * 8, bw * 8]"""
    bh, bw, _ = coefs.shape
    qn = np.zeros(64, dtype=np.int64)
    qn[ZIGZAG] = q
    x = (coefs.astype(np.int64) * qn).reshape(bh, bw, 8, 8)                   # [.., row, column]
    ws = np.stack(_idct_1d([x[:, :, r, :] for r in range(8)], 11, descale_bias), axis=2)    # pass 1 down the columns
    o = np.stack(_idct_1d([ws[:, :, :, c] for c in range(8)], 18, descale_bias), axis=3)
    o = np.clip(o + 128, 0, 255).astype(np.uint8)
    return o.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p, fancy=True):
    p = p.astype(np.int32)
    n = p.shape[1]
    out = np.repeat(p, 2, axis=1)
    if fancy and n > 2:
        left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
        right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p, fancy=True):
    p = p.astype(np.int32)
    h, n = p.shape
    if not fancy or n <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    dn = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.zeros((2 * h, 2 * n), dtype=np.int32)
    for par, other in ((0, up), (1, dn)):
        s = 3 * p + other
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[par::2, 0::2], out[par::2, 1::2] = even, odd
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct(hdr, coefs, fancy=True, descale_bias=0):
    W, H, comps = hdr["W"], hdr["H"], hdr["comps"]
    planes = [idct_plane(cf, c["q"], descale_bias)[:c["ph"], :c["pw"]] for cf, c in zip(coefs, comps)]
    if len(comps) == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    y = planes[0].astype(np.int32)[:H, :W]
    if (hdr["hmax"], hdr["vmax"]) == (2, 2):
        cb, cr = (upsample_h2v2(p, fancy)[:H, :W] for p in planes[1:])
    elif (hdr["hmax"], hdr["vmax"]) == (2, 1):
        cb, cr = (upsample_h2v1(p, fancy)[:H, :W] for p in planes[1:])
    else:
        cb, cr = (p.astype(np.int32) for p in planes[1:])
    cb, cr = cb - 128, cr - 128
    half = 1 << 15
    r = y + ((_fix(1.402) * cr + half) >> 16)
    b = y + ((_fix(1.772) * cb + half) >> 16)
    g = y + ((-_fix(0.34414) * cb + half - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_rgb(buf, **kw):
    hdr = parse(buf)
    if hdr is None:
        return None
    coefs, _ = sequential_coefficients(hdr)
    return reconstruct(hdr, coefs, **kw)


# ---------------------------------------------------------------------------------------------------------------- test files
def photo(w, h, seed):
    """photo-like frame: a smooth field plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        f = rng.uniform(0.01, 0.08, size=4)
        ph = rng.uniform(0, 6.28, size=2)
        img[:, :, c] = 128 + 70 * np.sin(xx * f[0] + yy * f[1] + ph[0]) + 40 * np.cos(xx * f[2] - yy * f[3] + ph[1])
    img += rng.normal(0, 12, size=img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(arr, quality, sampling, gray=False, **kw):
    import io

    from PIL import Image
    im = Image.fromarray(arr)
    if gray:
        im = im.convert("L")
    bio = io.BytesIO()
    if gray:
        im.save(bio, "JPEG", quality=quality, **kw)
    else:
        im.save(bio, "JPEG", quality=quality, subsampling=sampling, **kw)
    return bio.getvalue()


def pillow_rgb(buf):
    import io

    from PIL import Image
    return np.array(Image.open(io.BytesIO(buf)).convert("RGB"))


MATRIX_SIZES = [(1, 1), (7, 4), (8, 8), (9, 3), (16, 16), (17, 9), (40, 6), (13, 17), (33, 31), (5, 64)]      # (W, H)
MATRIX_SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "gray"]
MATRIX_QUALITIES = [5, 50, 90, 100]
MATRIX_VARIANTS = [{}, {"optimize": True}, {"restart_marker_blocks": 1}]


def matrix():
    """the 480 small files: 10 sizes x 4 samplings x 4 qualities x {plain, optimize, restart every block}"""
    for si, (w, h) in enumerate(MATRIX_SIZES):
        frame = photo(w, h, 100 + si)
        for samp in MATRIX_SAMPLINGS:
            for q in MATRIX_QUALITIES:
                for vi, kw in enumerate(MATRIX_VARIANTS):
                    yield (f"{w}x{h}-{samp}-q{q}-v{vi}", encode(frame, q, samp if samp != "gray" else None, gray=samp == "gray", **kw))


def big_files():
    """(name, bytes): 96 wide x 128 high, q95 4:4:4 / q75 4:2:0 / q75 4:2:0 with a restart marker every 3 MCU rows' worth of blocks"""
    f = photo(96, 128, 7)
    return [("q95-444", encode(f, 95, "4:4:4")), ("q75-420", encode(f, 75, "4:2:0")),
            ("q75-420-rst3", encode(f, 75, "4:2:0", restart_marker_blocks=3))]


_CACHE = {}


def all_files():
    """the matrix and the three larger files, encoded once per process"""
    if "files" not in _CACHE:
        _CACHE["files"] = list(matrix()) + big_files()
    return _CACHE["files"]


def reference_of(index):
    """(header, sequential coefficients, status) of all_files()[index], computed once and never modified by its users"""
    key = ("ref", index)
    if key not in _CACHE:
        hdr = parse(all_files()[index][1])
        coefs, status = sequential_coefficients(hdr)
        for c in coefs:
            c.setflags(write=False)
        _CACHE[key] = (hdr, coefs, status)
    return _CACHE[key]
