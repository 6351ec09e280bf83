"""The baseline JPEG decoder of the MJPG playback, restated literally: the oracle of
tests/test_jpeg_decode_cpu.py and tests/test_gpu_jpeg_decode.py. A stream of the accepted kind (SOF0, 8 bit, three
components at 2 x 2 / 1 x 1 / 1 x 1, one interleaved scan, any DQT / DHT / DRI) becomes a (h, w, 3) u8 BGR picture
and a status; the pixel arithmetic (dequantise, the slow-integer IDCT, the h2v2 triangle filter, the table colour
conversion) is libjpeg-turbo's default path, int32 with arithmetic shifts, and equals Pillow byte for byte
(tests/golden/jpeg_decode.npz).

    parse(stream)            the header: Header, or JpegError for anything outside the contract
    decode_scan(hdr, stream) the entropy walk: coefficients (MCU rows, MCUs a row, 6, 64) int16 zig-zag, status
    pixels(coef, hdr)        the picture of those coefficients
    decode(stream)           (picture, status)

Also a minimal RIFF reader (avi_index) the AVI tests compare svx.video.VideoCapture with."""
import struct

import numpy as np

import jpeg_numpy as jn

# the status of a frame: 0, or the largest of what its intervals met
OK, BAD_CODE, BAD_SIZE, BAD_RUN, RST_COUNT, RST_ORDER, NO_EOI = 0, 1, 2, 3, 4, 5, 6


class JpegError(ValueError):
    """A stream outside the contract (the host parser's SV_E_ARG)."""


class Header:
    def __init__(self):
        self.h = self.w = 0
        self.ri = 0               # the restart interval in MCUs (0: none)
        self.quant = None         # (3, 64) int32 by component, zig-zag order
        self.dc = [None] * 3      # (bits, vals) by component
        self.ac = [None] * 3
        self.scan_at = 0          # the first byte of the entropy-coded segment

    @property
    def mcus(self):
        return (-(-self.h // 16)) * (-(-self.w // 16))

    @property
    def intervals(self):
        return -(-self.mcus // self.ri) if self.ri else 1


_UNSUPPORTED = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential",
                0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic",
                0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless", 0xCD: "arithmetic differential",
                0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless",
                0xCC: "arithmetic conditioning (DAC)"}


def parse(stream):
    s = bytes(stream)
    n = len(s)
    if n < 4 or s[0] != 0xFF or s[1] != 0xD8:
        raise JpegError("no SOI")
    hdr = Header()
    qt, dht, sof = {}, {}, None
    i = 2
    while True:
        if i + 4 > n:
            raise JpegError("the header runs past the buffer")
        if s[i] != 0xFF:
            raise JpegError(f"no marker at byte {i}")
        m = s[i + 1]
        if m == 0xFF:            # a fill byte
            i += 1
            continue
        ln = s[i + 2] << 8 | s[i + 3]
        if ln < 2 or i + 2 + ln > n:
            raise JpegError(f"segment {m:#x} runs past the buffer")
        p = s[i + 4:i + 2 + ln]
        if m in _UNSUPPORTED:
            raise JpegError(_UNSUPPORTED[m] + " coding")
        if m == 0xC0:
            if sof is not None:
                raise JpegError("two SOF0")
            if len(p) < 6 or p[0] != 8:
                raise JpegError(f"{p[0] if p else '?'}-bit samples")
            hdr.h, hdr.w, nc = p[1] << 8 | p[2], p[3] << 8 | p[4], p[5]
            if nc != 3:
                raise JpegError(f"{nc} components")
            if len(p) != 6 + 3 * nc:
                raise JpegError("SOF0 length")
            sof = [(p[6 + 3 * k], p[7 + 3 * k], p[8 + 3 * k]) for k in range(3)]
            if [c[1] for c in sof] != [0x22, 0x11, 0x11]:
                raise JpegError("sampling factors other than 2x2, 1x1, 1x1 (4:2:0)")
            if any(c[2] > 3 for c in sof):
                raise JpegError("quantisation table id")
            if not (1 <= hdr.h <= 4096 and 1 <= hdr.w <= 4096):
                raise JpegError("1 <= h, w <= 4096")
        elif m == 0xDB:
            j = 0
            while j < len(p):
                if p[j] >> 4:
                    raise JpegError("16-bit DQT")
                if (p[j] & 15) > 3 or j + 65 > len(p):
                    raise JpegError("DQT")
                qt[p[j] & 15] = np.frombuffer(p[j + 1:j + 65], np.uint8).astype(np.int32)
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(p):
                if j + 17 > len(p):
                    raise JpegError("DHT")
                tc, th = p[j] >> 4, p[j] & 15
                bits = list(p[j + 1:j + 17])
                cnt = sum(bits)
                if tc > 1 or th > 1 or cnt > 256 or j + 17 + cnt > len(p):
                    raise JpegError("DHT")
                code = 0
                for ln_ in range(1, 17):          # the codes fit their lengths
                    code += bits[ln_ - 1]
                    if code > (1 << ln_):
                        raise JpegError("DHT code lengths")
                    code <<= 1
                dht[(tc, th)] = (bits, list(p[j + 17:j + 17 + cnt]))
                j += 17 + cnt
        elif m == 0xDD:
            if len(p) != 2:
                raise JpegError("DRI")
            hdr.ri = p[0] << 8 | p[1]
        elif m == 0xDA:
            if sof is None:
                raise JpegError("SOS before SOF0")
            if len(p) != 10 or p[0] != 3:
                raise JpegError("a scan of other than three components")
            for k in range(3):
                if p[1 + 2 * k] != sof[k][0]:
                    raise JpegError("scan components out of order")
                td, ta = p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15
                if td > 1 or ta > 1:
                    raise JpegError("Huffman table id")
                hdr.dc[k], hdr.ac[k] = (0, td), (1, ta)
            if (p[7], p[8], p[9]) != (0, 63, 0):
                raise JpegError("a scan that is not Ss = 0, Se = 63, Ah = Al = 0")
            hdr.scan_at = i + 2 + ln
            break
        elif m in (0xD9,):
            raise JpegError("EOI before SOS")
        elif 0xD0 <= m <= 0xD7 or m == 0x01 or m == 0xD8:
            raise JpegError(f"marker {m:#x} in the header")
        elif m == 0xDC or m == 0xDE or m == 0xDF:
            raise JpegError(f"marker {m:#x} (DNL / hierarchical)")
        # APPn, COM and the rest: skipped
        i += 2 + ln
    if not dht:                  # MJPG frames of other writers: the Annex K tables
        dht = {(0, 0): jn.DC_L, (1, 0): jn.AC_L, (0, 1): jn.DC_C, (1, 1): jn.AC_C}
    q = []
    for k in range(3):
        if sof[k][2] not in qt:
            raise JpegError("a quantisation table that no DQT defines")
        q.append(qt[sof[k][2]])
        for tabs in (hdr.dc, hdr.ac):
            if tabs[k] not in dht:
                raise JpegError("a Huffman table that no DHT defines")
            tabs[k] = dht[tabs[k]]
    hdr.quant = np.stack(q)
    return hdr


def intervals_of(hdr, stream):
    """[(first byte, end)] of the intervals and the scan's status: RSTn positions in order, up to the first other
    marker (EOI)."""
    s = bytes(stream)
    a = np.frombuffer(s, np.uint8)[hdr.scan_at:]
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    nxt = a[ff + 1] if ff.size else np.zeros(0, np.uint8)
    other = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)) & (nxt != 0xFF)]
    end = int(other[0]) if other.size else int(a.size)
    status = OK if other.size else NO_EOI
    rst = [(int(p), int(c)) for p, c in zip(ff, nxt) if 0xD0 <= c <= 0xD7 and p < end]
    n = hdr.intervals
    bad = OK
    if len(rst) != n - 1:
        bad = RST_COUNT
    if any(c - 0xD0 != (k & 7) for k, (_, c) in enumerate(rst)):
        bad = RST_ORDER
    if bad:                       # no intervals to decode
        return [], max(status, bad)
    starts = [0] + [p + 2 for p, _ in rst]
    ends = [p for p, _ in rst] + [end]
    return [(hdr.scan_at + a_, hdr.scan_at + b_) for a_, b_ in zip(starts, ends)], status


def _lookup(bits, vals):
    """The 16-bit window -> (length, symbol) table of a DHT; length 0 where no code matches."""
    ln_tab = np.zeros(1 << 16, np.uint8)
    sym_tab = np.zeros(1 << 16, np.uint8)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            lo = code << (16 - ln)
            ln_tab[lo:lo + (1 << (16 - ln))] = ln
            sym_tab[lo:lo + (1 << (16 - ln))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return ln_tab.tolist(), sym_tab.tolist()


def _unstuff(seg):
    """The interval's data bytes: 0xFF 0x00 -> 0xFF; anything else behind a 0xFF ends the data."""
    a = np.frombuffer(seg, np.uint8)
    ff = np.flatnonzero(a == 0xFF)
    keep = np.ones(a.size, bool)
    for p in ff:
        if p + 1 < a.size and a[p + 1] == 0:
            keep[p + 1] = False
        else:                     # a stray marker (or a 0xFF as the last byte, its partner cut off)
            if p + 1 < a.size:
                keep[p:] = False
            break
    return a[keep]


def decode_interval(seg, hdr, mcus, tabs):
    """(mcus, 6, 64) int16 zig-zag coefficients of one interval's bytes, and its status. Bits past the end are
    zeros; what follows an error stays zero."""
    data = _unstuff(seg)
    pad = np.concatenate([data, np.zeros(8, np.uint8)]).astype(np.uint64)
    win = ((pad[:-4] << np.uint64(32)) | (pad[1:-3] << np.uint64(24)) | (pad[2:-2] << np.uint64(16)) |
           (pad[3:-1] << np.uint64(8)) | pad[4:]).tolist()          # 40 bits from every byte
    nwin = len(win)
    out = np.zeros((mcus, 6, 64), np.int64)
    pos = 0

    def peek(n):                  # n <= 16 bits at pos
        i = pos >> 3
        if i >= nwin:
            return 0
        return (win[i] >> (40 - (pos & 7) - n)) & ((1 << n) - 1)

    pred = [0, 0, 0]
    comp = (0, 0, 0, 0, 1, 2)
    for m in range(mcus):
        for k in range(6):
            c = comp[k]
            dln, dsym = tabs[("dc", c)]
            aln, asym = tabs[("ac", c)]
            v = peek(16)
            ln = dln[v]
            if ln == 0:
                return out, BAD_CODE
            pos += ln
            s = dsym[v]
            if s > 11:
                return out, BAD_SIZE
            diff = 0
            if s:
                diff = peek(s)
                pos += s
                if diff < (1 << (s - 1)):
                    diff -= (1 << s) - 1
            pred[c] += diff
            blk = out[m, k]
            blk[0] = pred[c]
            z = 1
            while z < 64:
                v = peek(16)
                ln = aln[v]
                if ln == 0:
                    return out, BAD_CODE
                pos += ln
                rs = asym[v]
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break
                    if z + 15 > 63:
                        return out, BAD_RUN
                    z += 16
                    continue
                z += r
                if z > 63:
                    return out, BAD_RUN
                if s > 10:
                    return out, BAD_SIZE
                val = peek(s)
                pos += s
                if val < (1 << (s - 1)):
                    val -= (1 << s) - 1
                blk[z] = val
                z += 1
    return out, OK


def decode_scan(hdr, stream):
    """Coefficients (MCU rows, MCUs a row, 6, 64) int16 in zig-zag order, and the frame's status."""
    s = bytes(stream)
    mr, mc = -(-hdr.h // 16), -(-hdr.w // 16)
    total = mr * mc
    coef = np.zeros((total, 6, 64), np.int64)
    ivals, status = intervals_of(hdr, s)
    if not ivals:
        return coef.reshape(mr, mc, 6, 64).astype(np.int16), status
    cache, tabs = {}, {}
    for c in range(3):
        for kind, t in (("dc", hdr.dc[c]), ("ac", hdr.ac[c])):
            key = (tuple(t[0]), tuple(t[1]))
            if key not in cache:
                cache[key] = _lookup(*t)
            tabs[(kind, c)] = cache[key]
    per = hdr.ri if hdr.ri else total
    for k, (a, b) in enumerate(ivals):
        m0 = k * per
        n = min(per, total - m0)
        got, st = decode_interval(s[a:b], hdr, n, tabs)
        coef[m0:m0 + n] = got
        status = max(status, st)
    return coef.reshape(mr, mc, 6, 64).astype(np.int16), status


# ---- pixels ----------------------------------------------------------------------------------------------------
def _idct_pass(c, n):
    """jidctint's one-dimensional pass along the last axis of c (.., 8) int32, descaled by n bits."""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2 = z1 - c[6] * 15137
    t3 = z1 + c[2] * 6270
    t0 = (c[0] + c[4]) << 13
    t1 = (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (n - 1)
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(v + r) >> n for v in o], axis=-1)


def idct(blocks):
    """(.., 8, 8) int32 dequantised coefficients, natural order -> samples 0..255."""
    with np.errstate(over="ignore"):
        d = blocks.astype(np.int32)
        d = np.swapaxes(_idct_pass(np.swapaxes(d, -1, -2), 11), -1, -2)    # columns
        d = _idct_pass(d, 18)                                              # rows
        return np.clip(d + 128, 0, 255)


def _plane(samples):
    """(rows, cols, 8, 8) blocks -> (8 rows, 8 cols)."""
    r, c = samples.shape[:2]
    return samples.swapaxes(1, 2).reshape(8 * r, 8 * c)


def upsample(c):
    """The h2v2 triangle filter ("fancy upsampling") with the edges repeated: (ch, cw) -> (2 ch, 2 cw) int32."""
    c = c.astype(np.int32)
    up, dn = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    s = np.empty((2 * c.shape[0], c.shape[1]), np.int32)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + dn
    lf, rt = np.hstack([s[:, :1], s[:, :-1]]), np.hstack([s[:, 1:], s[:, -1:]])
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int32)
    out[:, 0::2], out[:, 1::2] = (3 * s + lf + 8) >> 4, (3 * s + rt + 7) >> 4
    return out


def pixels(coef, hdr):
    """coef (MCU rows, MCUs a row, 6, 64) zig-zag, quantised -> (h, w, 3) u8 BGR."""
    h, w = hdr.h, hdr.w
    mr, mc = coef.shape[:2]
    nat = np.zeros((mr, mc, 6, 64), np.int32)
    comp = (0, 0, 0, 0, 1, 2)
    for k in range(6):
        nat[:, :, k, jn.ZIGZAG] = coef[:, :, k].astype(np.int32) * hdr.quant[comp[k]][None, None, :]
    smp = idct(nat.reshape(mr, mc, 6, 8, 8))
    yb = np.zeros((2 * mr, 2 * mc, 8, 8), np.int32)
    for k in range(4):
        yb[k >> 1::2, k & 1::2] = smp[:, :, k]
    y = _plane(yb)[:h, :w]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    cb = upsample(_plane(smp[:, :, 4])[:ch, :cw])[:h, :w] - 128
    cr = upsample(_plane(smp[:, :, 5])[:ch, :cw])[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


def decode(stream):
    """(picture, status) of a stream; JpegError for one outside the contract."""
    hdr = parse(stream)
    coef, status = decode_scan(hdr, stream)
    return pixels(coef, hdr), status


def pixels_of_picture(bgr, quality):
    """What decoding jn.encode(bgr, quality) gives, without the entropy coder (the 272 x 1024 cases in a moment)."""
    hdr = Header()
    hdr.h, hdr.w = bgr.shape[:2]
    ql, qc = jn.quant_table(jn.K1, quality)[jn.ZIGZAG], jn.quant_table(jn.K2, quality)[jn.ZIGZAG]
    hdr.quant = np.stack([ql, qc, qc])
    return pixels(jn.coefficients(bgr, quality), hdr)


def strip_dht(stream):
    """The stream without its DHT segments (MJPG frames of other writers rely on the Annex K tables)."""
    s = bytes(stream)
    out, i = bytearray(s[:2]), 2
    while True:
        m, n = s[i + 1], s[i + 2] << 8 | s[i + 3]
        if m != 0xC4:
            out += s[i:i + 2 + n]
        i += 2 + n
        if m == 0xDA:
            return bytes(out) + s[i:]


# ---- AVI -------------------------------------------------------------------------------------------------------
def avi_index(buf):
    """(frames as bytes, w, h, rate, scale) of a RIFF AVI by a plain walk of its lists."""
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI "
    i, frames, info = 12, [], {}
    while i + 8 <= len(buf):
        cc, n = struct.unpack_from("<4sI", buf, i)
        if cc == b"LIST" and buf[i + 8:i + 12] == b"hdrl":
            j = i + 12
            while j < i + 8 + n:
                c2, m = struct.unpack_from("<4sI", buf, j)
                if c2 == b"LIST":
                    j += 12
                    continue
                if c2 == b"strh":
                    info["scale"], info["rate"] = struct.unpack_from("<II", buf, j + 8 + 20)
                if c2 == b"strf":
                    info["w"], info["h"] = struct.unpack_from("<ii", buf, j + 8 + 4)
                j += 8 + m + (m & 1)
        if cc == b"LIST" and buf[i + 8:i + 12] == b"movi":
            frames = jn.avi_frames(buf)
        i += 8 + n + (n & 1)
    return frames, info["w"], info["h"], info["rate"], info["scale"]


# ---- malformed scans and refused headers (shared by the CPU and GPU tests) --------------------------------------
def rst_positions(stream):
    hdr = parse(stream)
    s = bytes(stream)
    return [i for i in range(hdr.scan_at, len(s) - 1) if s[i] == 0xFF and 0xD0 <= s[i + 1] <= 0xD7]


def malformed(stream):
    """{name: (stream, status)} of a valid stream with at least three intervals and the Annex K tables: a scan cut in
    the middle, the last RST missing, two RST indices swapped, a code outside the table."""
    s = bytes(stream)
    hdr, rst = parse(s), rst_positions(s)
    assert len(rst) >= 2
    cut = s[:hdr.scan_at + (len(s) - hdr.scan_at) // 2]
    gone = s[:rst[-1]] + s[rst[-1] + 2:]
    swap = bytearray(s)
    swap[rst[0] + 1], swap[rst[1] + 1] = swap[rst[1] + 1], swap[rst[0] + 1]
    code = bytearray(s)
    code[hdr.scan_at:hdr.scan_at + 4] = b"\xff\x00\xff\x00"       # sixteen 1-bits: no DC code
    return {"cut": (cut, None), "missing-rst": (gone, RST_COUNT), "swapped-rst": (bytes(swap), RST_ORDER),
            "bad-code": (bytes(code), BAD_CODE)}


def _patch_segment(stream, marker, fn):
    """The stream with fn(payload) -> payload applied to its first segment `marker` (the length field follows)."""
    s = bytes(stream)
    i = 2
    while True:
        m, n = s[i + 1], s[i + 2] << 8 | s[i + 3]
        if m == marker:
            p = bytes(fn(bytearray(s[i + 4:i + 2 + n])))
            return s[:i + 2] + (len(p) + 2).to_bytes(2, "big") + p + s[i + 2 + n:]
        assert m != 0xDA, "no such segment"
        i += 2 + n


def _set(idx, val):
    def fn(p):
        p[idx] = val
        return p
    return fn


def refused(stream):
    """{name: (stream, a word of the refusal)}: one stream of every unsupported kind, made from a valid one."""
    s = bytes(stream)
    sof = s.index(b"\xff\xc0")
    out = {}
    for name, m, word in (("progressive", 0xC2, "progressive"), ("arithmetic", 0xC9, "arithmetic"),
                          ("extended", 0xC1, "extended"), ("lossless", 0xC3, "lossless")):
        out[name] = (s[:sof + 1] + bytes([m]) + s[sof + 2:], word)
    out["12-bit"] = (_patch_segment(s, 0xC0, _set(0, 12)), "8 bit")
    out["1-component"] = (_patch_segment(s, 0xC0, lambda p: p[:5] + bytes([1]) + p[6:9]), "component")
    out["4-components"] = (_patch_segment(s, 0xC0, lambda p: p[:5] + bytes([4]) + p[6:] + bytes([4, 0x11, 1])),
                           "component")
    out["4:2:2"] = (_patch_segment(s, 0xC0, _set(7, 0x21)), "sampling")
    out["4:4:4"] = (_patch_segment(s, 0xC0, _set(7, 0x11)), "sampling")
    out["several-scans"] = (_patch_segment(s, 0xDA, lambda p: bytes([1]) + p[1:3] + p[7:]), "scan")
    out["spectral"] = (_patch_segment(s, 0xDA, _set(8, 5)), "scan")
    out["16-bit-dqt"] = (_patch_segment(s, 0xDB, lambda p: bytes([0x10 | p[0]]) + p[1:] + p[1:]), "16-bit")
    dqt = s.index(b"\xff\xdb")
    out["length"] = (s[:dqt + 2] + b"\xff\xf0" + s[dqt + 4:], "past the buffer")
    out["no-soi"] = (b"\x00\x00" + s[2:], "SOI")
    out["zero-height"] = (_patch_segment(s, 0xC0, lambda p: p[:1] + b"\0\0" + p[3:]), "4096")
    return out
