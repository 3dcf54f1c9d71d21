"""Host side of the GPU JPEG decode (--gpu_jpeg; DESIGN.md §4.7 "JPEG decode"; kernels: csrc/jpeg.hip).

The reference decodes every image with PIL inside `__getitem__` on one host core (data.py:848-860).  Here a DataLoader worker only
reads the file, parses its headers (`parse_jpeg`) and removes the byte stuffing; the entropy decode, the IDCT, the chroma upsampling
and the colour conversion run on the GPU and give the frame Pillow gives, byte for byte.  Files outside the supported class make
`parse_jpeg` return None and are decoded by Pillow on the host as before; an image whose scan turns out to be damaged comes back
from the GPU with a non-zero status and is decoded by Pillow from the kept bytes (`decode_with_fallback`), and a pair whose image
Pillow cannot read either is dropped from the batch (`drop_rows`), which is the reference's rule for an image that fails to load.

Supported: sequential Huffman JPEG with 8-bit samples (SOF0, SOF1), one interleaved scan (Ss 0, Se 63, Ah = Al = 0), one component,
or three that libjpeg reads as YCbCr (JFIF, or Adobe transform 1, or ids 1 2 3) with luma sampling 1x1 / 2x1 / 2x2 and 1x1 chroma,
any restart interval, 8-bit quantisation tables, at most MAX_PIXELS pixels.

Byte unstuffing and the cut at the restart markers happen here, vectorised, in the worker process: the device gets segments that
start at multiples of four bytes and hold entropy-coded bits only.
"""
import numpy as np
import torch

MAX_PIXELS = 1 << 25            # 33.5 Mpixel: at most 6 bytes of coefficients per pixel, so one image always fits the workspace below
MAX_SCAN_BYTES = 1 << 27        # bit positions stay far inside int32
COEF_CHUNK_BYTES = 256 << 20    # coefficient workspace of one chunk of a batch (int16); the planes take half as much again
GUARD = 64                      # int16 elements the kernels leave untouched around every component grid (csrc/jpeg.hip JPEG_GUARD)
TABLE_BYTES, TABLES_PER_IMAGE = 1424, 6
DESC_WORDS = 16
(D_W, D_H, D_NCOMP, D_HS, D_VS, D_MX, D_MY, D_RI, D_NSEG, D_SEG0, D_NPIECES, D_PIECE0, D_MAXSEGPIECES, D_COEF, D_PLANE, D_OUT) = range(16)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63], dtype=np.int64)


_BLOBS = {}


def huffman_blob(counts, values, is_dc):
    """Device form of one DHT table (TABLE_BYTES bytes): uint16 look[512] (9-bit look-ahead: length << 8 | symbol, 0 = the code is
    longer), int32 maxcode[18] (-1 = no code of that length), int32 valoff[17] (index of a length's first symbol minus its first
    code), uint8 symbols[256].  None for a table libjpeg would refuse.  Most files carry the same few tables: built once each."""
    key = (bytes(counts), bytes(values), is_dc)
    if key in _BLOBS:
        return _BLOBS[key]
    blob = _huffman_blob(counts, values, is_dc)
    if len(_BLOBS) >= 256:
        _BLOBS.clear()
    _BLOBS[key] = blob
    return blob


def _huffman_blob(counts, values, is_dc):
    nv = int(sum(counts))
    if nv > 256 or nv != len(values) or nv == 0:
        return None
    if is_dc and any(v > 15 for v in values):
        return None
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(17, dtype=np.int32)
    code = k = 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n:
            if code + n > (1 << length):
                return None                                    # over-subscribed
            valoff[length] = k - code
            code += n
            k += n
            maxcode[length] = code - 1
        code <<= 1
    # canonical codes come in increasing order, so the look-ahead entries of the codes of at most 9 bits fill the table from 0 on
    lengths = np.repeat(np.arange(1, 17), counts)
    short = lengths <= 9
    entries = np.repeat(((lengths[short] << 8) | np.asarray(values, dtype=np.int64)[short]).astype(np.uint16), 1 << (9 - lengths[short]))
    look = np.zeros(512, dtype=np.uint16)
    look[:len(entries)] = entries
    blob = np.zeros(TABLE_BYTES, dtype=np.uint8)
    blob[0:1024] = look.view(np.uint8)
    blob[1024:1096] = maxcode.view(np.uint8)
    blob[1096:1164] = valoff.view(np.uint8)
    blob[1164:1164 + nv] = np.asarray(values, dtype=np.uint8)
    blob.setflags(write=False)
    return blob


class JpegPlan:
    """What the device needs besides the bits: geometry, tables, and the unstuffed scan cut into restart segments."""
    __slots__ = ("width", "height", "ncomp", "hs", "vs", "mx", "my", "ri", "qt", "tables", "scan", "seg_off", "seg_len")

    def __getstate__(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __setstate__(self, state):
        for n, v in zip(self.__slots__, state):
            setattr(self, n, v)

    @property
    def sampling(self):
        """per component (h, v)"""
        return [(self.hs, self.vs)] + [(1, 1)] * (self.ncomp - 1)

    @property
    def mcus(self):
        return self.mx * self.my

    @property
    def blocks(self):
        """blocks of each component's MCU-padded grid"""
        return [self.mcus * self.hs * self.vs] + [self.mcus] * (self.ncomp - 1)

    def grid(self, c):
        """(block rows, block columns) of component c"""
        return (self.my * self.vs, self.mx * self.hs) if c == 0 else (self.my, self.mx)

    @property
    def coef_elements(self):
        """int16 elements of this image in the coefficient workspace, guards included"""
        return sum(self.blocks) * 64 + (self.ncomp + 1) * GUARD


def _unstuff(raw, zeros):
    """raw without the bytes at the (sorted) positions `zeros`: the slices between them, joined"""
    if not zeros:
        return bytes(raw)
    return b"".join([raw[s:e] for s, e in zip([0] + [z + 1 for z in zeros], zeros + [len(raw)])])


def _split_scan(raw, stuffed, rst, nseg):
    """Entropy-coded bytes between SOS and the next marker, the positions of the FFs of their FF 00 pairs and of their RSTn markers
    -> (buffer with every restart segment unstuffed and starting at a multiple of 4, offsets [nseg], lengths [nseg])."""
    if len(rst) == 0:
        segs = [_unstuff(raw, (stuffed + 1).tolist())]
    else:
        first = [0] + (rst + 2).tolist()
        last = rst.tolist() + [len(raw)]
        at = [0] + np.searchsorted(stuffed, rst).tolist() + [len(stuffed)]
        segs = [_unstuff(raw[first[i]:last[i]], (stuffed[at[i]:at[i + 1]] + (1 - first[i])).tolist()) for i in range(len(first))]
    lens = np.zeros(max(nseg, len(segs)), dtype=np.int64)
    lens[:len(segs)] = [len(x) for x in segs]
    padded = (lens + 3) & ~3
    offs = np.cumsum(padded) - padded
    if len(segs) == 1:
        buf = segs[0] + b"\0" * (int(padded[0]) - len(segs[0]))
    else:
        buf = b"".join([x + b"\0" * (-len(x) & 3) for x in segs])
    out = np.frombuffer(buf or b"\0\0\0\0", dtype=np.uint8)
    return out, offs[:nseg].astype(np.int32), lens[:nseg].astype(np.int32)


def parse_jpeg(buf):
    """File bytes (bytes / uint8 array) -> JpegPlan, or None for anything outside the supported class (module docstring)."""
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    n = len(a)
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        return None
    b = a.tobytes()
    qts, dht, sof, ri, jfif, adobe = {}, {}, None, 0, False, None
    pos = 2
    while True:                                                 # segment by segment, by their lengths
        if pos + 4 > n or b[pos] != 0xFF:
            return None
        m = b[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            pos += 2
            continue
        ln = (b[pos + 2] << 8) | b[pos + 3]
        if ln < 2 or pos + 2 + ln > n:
            return None
        seg = b[pos + 4:pos + 2 + ln]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                if seg[i] >> 4 or (seg[i] & 15) > 3 or i + 65 > len(seg):
                    return None
                qts[seg[i] & 15] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=i + 1)
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg) or (seg[i] >> 4) > 1 or (seg[i] & 15) > 3:
                    return None
                counts = list(seg[i + 1:i + 17])
                nv = sum(counts)
                if i + 17 + nv > len(seg):
                    return None
                dht[(seg[i] >> 4, seg[i] & 15)] = (counts, list(seg[i + 17:i + 17 + nv]))
                i += 17 + nv
        elif m in (0xC0, 0xC1):
            if sof is not None or len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                return None
            sof = seg
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None                                         # progressive, lossless, arithmetic, hierarchical
        elif m == 0xDD:
            if len(seg) < 2:
                return None
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m in (0xDC, 0xD9):
            return None                                         # DNL; EOI before any scan
        elif m == 0xDA:
            sos = seg
            start = pos + 2 + ln
            break
        pos += 2 + ln
    if sof is None or sof[0] != 8:
        return None
    H, W, nc = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    if H == 0 or W == 0 or W * H > MAX_PIXELS or nc not in (1, 3):
        return None
    comps = [(sof[6 + 3 * c], sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15, sof[8 + 3 * c]) for c in range(nc)]
    if len(sos) != 4 + 2 * nc or sos[0] != nc or tuple(sos[1 + 2 * nc:]) != (0, 63, 0):
        return None
    if [sos[1 + 2 * c] for c in range(nc)] != [c[0] for c in comps]:
        return None
    if nc == 3:
        if adobe is not None:
            if adobe != 1:
                return None
        elif not jfif and [c[0] for c in comps] != [1, 2, 3]:
            return None                                         # libjpeg guesses RGB (or warns) here: leave it to libjpeg
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
    p = JpegPlan()
    p.width, p.height, p.ncomp = W, H, nc
    p.hs, p.vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)      # a single component is never interleaved: its factors do not matter
    p.mx, p.my = -(-W // (8 * p.hs)), -(-H // (8 * p.vs))
    p.ri = ri if ri else p.mx * p.my
    p.qt = np.zeros((3, 64), dtype=np.uint8)
    p.tables = np.zeros((TABLES_PER_IMAGE, TABLE_BYTES), dtype=np.uint8)
    for c in range(nc):
        q = qts.get(comps[c][3])
        td, ta = sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15
        if q is None or (0, td) not in dht or (1, ta) not in dht:
            return None
        p.qt[c, ZIGZAG] = q
        dc, ac = huffman_blob(*dht[(0, td)], True), huffman_blob(*dht[(1, ta)], False)
        if dc is None or ac is None:
            return None
        p.tables[2 * c], p.tables[2 * c + 1] = dc, ac
    # end of the scan: the first FF followed by anything but 00 or RSTn (a last byte FF of a cut file is data)
    scan = a[start:]
    if len(scan) < 1 or len(scan) > MAX_SCAN_BYTES:
        return None
    ff = np.flatnonzero(scan == 0xFF)
    if len(ff) and ff[-1] == len(scan) - 1:
        ff = ff[:-1]
    nxt = scan[ff + 1]
    end = len(scan)
    stop = np.flatnonzero((nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)))
    if len(stop):
        if nxt[stop[0]] != 0xD9:
            return None                                         # fill bytes, a second scan, DNL, ...
        end, ff, nxt = int(ff[stop[0]]), ff[:stop[0]], nxt[:stop[0]]
    if end < 1:
        return None
    rst = ff[nxt != 0]                                          # what is left besides the stuffed zeros are the RSTn markers
    if len(rst) and not np.array_equal(nxt[nxt != 0] - 0xD0, np.arange(len(rst)) & 7):
        return None                                             # out of sequence: libjpeg resynchronises, leave it to libjpeg
    split = _split_scan(memoryview(b)[start:start + end], ff[nxt == 0], rst, -(-(p.mx * p.my) // p.ri))
    p.scan, p.seg_off, p.seg_len = split
    return p


class JpegImage:
    """An undecoded sample for the GPU pipeline: the file's bytes (kept for the Pillow fallback), the plan, the transform's draw.
    Pickles as two byte arrays and a few small ones: a twentieth of the decoded frame for a typical photo."""
    __slots__ = ("data", "plan", "params")

    def __init__(self, data, plan, params):
        self.data, self.plan, self.params = data, plan, params

    def __getstate__(self):
        return (self.data, self.plan, self.params)

    def __setstate__(self, state):
        self.data, self.plan, self.params = state

    @property
    def flip(self):
        return bool(self.params.flip)


def pillow_decode(data):
    """uint8 tensor / bytes of a file -> uint8 [H, W, 3] tensor through Pillow (raises what Pillow raises)"""
    import io

    from PIL import Image
    raw = data.numpy().tobytes() if torch.is_tensor(data) else bytes(data)
    return torch.from_numpy(np.array(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8))


def _pack(arrays):
    """several host arrays -> one uint8 buffer (16-byte aligned sections) + the section offsets: one copy to the device"""
    offs, total = [], 0
    for x in arrays:
        offs.append(total)
        total += (x.nbytes + 15) & ~15
    buf = np.zeros(max(total, 16), dtype=np.uint8)
    for o, x in zip(offs, arrays):
        buf[o:o + x.nbytes] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    return buf, offs


class GpuJpegDecoder:
    """decode(items) -> (device uint8 [H, W, 3] frames, int32 status per image), JpegImage items (or bare JpegPlans) of any sizes.

    A batch is worked in chunks whose coefficients fit COEF_CHUNK_BYTES (an image alone always does: MAX_PIXELS); every chunk is one
    host-to-device copy, one ia_jpeg_entropy launch and the two launches of ia_jpeg_reconstruct, whatever the number of images.  The
    workspace (coefficients, planes, piece states) is allocated once at the largest size seen and reused:
      coefficients  <= COEF_CHUNK_BYTES           (800 x 800 4:2:0: 1.9 MB an image)
      planes        half the coefficient bytes
      piece states  40 bytes per piece of subseq_bits bits of scan (1024 bits: a third of the scan's bytes)
    """

    def __init__(self, device):
        self.device = torch.device(device)
        self._coef = self._planes = self._pieces = None
        self.last_rounds = None

    def _buffer(self, name, n, dtype):
        t = getattr(self, name)
        if t is None or t.numel() < n:
            t = torch.empty(max(n, 1), device=self.device, dtype=dtype)
            setattr(self, name, t)
        return t

    @staticmethod
    def chunks(plans):
        out, cur, size = [], [], 0
        for i, p in enumerate(plans):
            b = p.coef_elements * 2
            if cur and size + b > COEF_CHUNK_BYTES:
                out.append(cur)
                cur, size = [], 0
            cur.append(i)
            size += b
        if cur:
            out.append(cur)
        return out

    @staticmethod
    def layout(plans, subseq_bits):
        """Host tables of one chunk -> dict of numpy arrays + totals (no device work)."""
        n = len(plans)
        desc = np.zeros((n, DESC_WORDS), dtype=np.int32)
        seg_off, seg_len, seg_piece0, piece_seg, scans = [], [], [], [], []
        coef = plane = out = seg0 = piece0 = scan0 = 0
        for i, p in enumerate(plans):
            npieces = np.maximum(1, -(-(p.seg_len.astype(np.int64) * 8) // subseq_bits)).astype(np.int32)
            first = np.concatenate([[0], np.cumsum(npieces)[:-1]]).astype(np.int32)
            total = int(npieces.sum())
            desc[i] = (p.width, p.height, p.ncomp, p.hs, p.vs, p.mx, p.my, p.ri, len(p.seg_len), seg0, total, piece0, int(npieces.max()),
                       coef + GUARD, plane, out)
            seg_off.append(p.seg_off + scan0)
            seg_len.append(p.seg_len)
            seg_piece0.append(first)
            piece_seg.append(np.repeat(np.arange(len(npieces), dtype=np.int32), npieces))
            scans.append(p.scan)
            scan0 += len(p.scan)
            seg0 += len(p.seg_len)
            piece0 += total
            coef += p.coef_elements
            plane += (sum(p.blocks) * 64 + 15) & ~15
            out += p.width * p.height * 3
        return dict(desc=desc, scan=np.concatenate(scans), seg_off=np.concatenate(seg_off).astype(np.int32),
                    seg_len=np.concatenate(seg_len).astype(np.int32), seg_piece0=np.concatenate(seg_piece0),
                    piece_seg=np.concatenate(piece_seg), tables=np.stack([p.tables for p in plans]), qt=np.stack([p.qt for p in plans]),
                    coef_elements=coef, plane_bytes=plane, out_bytes=out, pieces=piece0)

    def _upload(self, lay):
        names = ("desc", "scan", "seg_off", "seg_len", "seg_piece0", "piece_seg", "tables", "qt")
        buf, offs = _pack([lay[k] for k in names])
        dev = torch.from_numpy(buf).to(self.device, non_blocking=True)
        base = dev.data_ptr()
        return dev, {k: base + o for k, o in zip(names, offs)}, buf.nbytes

    def launch_entropy(self, lay, ptrs, n, subseq_bits, fill=None):
        """ia_jpeg_entropy over an uploaded layout -> (coefficient buffer, int32 [2, n] = status and pass-B rounds, on the device)"""
        from .. import _lib
        from .._lib import check, stream_ptr
        coef = self._buffer("_coef", lay["coef_elements"], torch.int16)
        if fill is not None:
            coef.fill_(fill)
        pieces = self._buffer("_pieces", lay["pieces"] * 10, torch.int32)
        stat = torch.empty((2, n), device=self.device, dtype=torch.int32)
        check(_lib.load().ia_jpeg_entropy(ptrs["desc"], n, ptrs["scan"], ptrs["seg_off"], ptrs["seg_len"], ptrs["seg_piece0"], ptrs["piece_seg"],
                                          ptrs["tables"], pieces.data_ptr(), lay["pieces"], coef.data_ptr(), int(subseq_bits), stat[0].data_ptr(),
                                          stat[1].data_ptr(), stream_ptr()), "ia_jpeg_entropy")
        return coef, stat

    def entropy(self, plans, subseq_bits=1024, fill=None):
        """Entropy stage of one chunk.  Returns (coef int16 tensor over the chunk's coefficient layout, status / rounds [2, n], lay,
        device pointers, keep-alive).  `fill`: int16 value the coefficient buffer holds beforehand (tests look at the guards)."""
        lay = self.layout(plans, subseq_bits)
        dev, ptrs, lay["h2d_bytes"] = self._upload(lay)
        coef, stat = self.launch_entropy(lay, ptrs, len(plans), subseq_bits, fill)
        return coef, stat, lay, ptrs, dev

    def reconstruct(self, plans, coef, lay, ptrs):
        """Reconstruction stage of one chunk from device coefficients in the chunk layout -> list of uint8 [H, W, 3] views"""
        from .. import _lib
        from .._lib import check, stream_ptr
        planes = self._buffer("_planes", lay["plane_bytes"], torch.uint8)
        out = torch.empty(max(lay["out_bytes"], 1), device=self.device, dtype=torch.uint8)
        check(_lib.load().ia_jpeg_reconstruct(ptrs["desc"], len(plans), coef.data_ptr(), ptrs["qt"], planes.data_ptr(), out.data_ptr(), stream_ptr()),
              "ia_jpeg_reconstruct")
        frames, o = [], 0
        for p in plans:
            nb = p.width * p.height * 3
            frames.append(out[o:o + nb].view(p.height, p.width, 3))
            o += nb
        return frames

    def decode(self, items, subseq_bits=1024, fill=None):
        plans = [getattr(it, "plan", it) for it in items]
        frames, stats = [None] * len(plans), []
        for idxs in self.chunks(plans):
            sub = [plans[i] for i in idxs]
            coef, stat, lay, ptrs, dev = self.entropy(sub, subseq_bits, fill)
            for i, f in zip(idxs, self.reconstruct(sub, coef, lay, ptrs)):
                frames[i] = f
            stats.append(stat)
            del dev
        st = torch.cat(stats, dim=1).cpu().numpy()               # the one read-back of the batch (it also ends the use of the workspace)
        self.last_rounds = st[1]
        return frames, st[0]


def decode_with_fallback(decoder, items):
    """JpegImage items -> list of uint8 [H, W, 3] frames (device tensors; host tensors for the ones Pillow had to decode), None where
    Pillow could not read the file either."""
    frames, status = decoder.decode(items)
    for i in np.flatnonzero(status):
        try:
            frames[i] = pillow_decode(items[i].data)
        except Exception:
            frames[i] = None
    return frames


def drop_rows(batch, keep):
    """The reference drops a pair whose image fails to load (data.py:44, :84).  With the decode on the GPU that is only known after
    the collate, so the rows are dropped here: `keep` (bools, one per row) applied to every element of the batch - tensors and lists
    row by row, RawImageBatch-like objects through their `items`, None left alone."""
    keep = [bool(k) for k in keep]
    if all(keep):
        return batch
    idx = [i for i, k in enumerate(keep) if k]

    def cut(t):
        if t is None:
            return None
        if torch.is_tensor(t):
            if t.dim() == 0 or t.shape[0] != len(keep):
                return t
            return t[torch.as_tensor(idx, dtype=torch.long, device=t.device)]
        if hasattr(t, "items") and not isinstance(t, dict):
            return type(t)([t.items[i] for i in idx])
        if isinstance(t, (list, tuple)) and len(t) == len(keep):
            return type(t)(t[i] for i in idx)
        return t

    return tuple(cut(t) for t in batch)
