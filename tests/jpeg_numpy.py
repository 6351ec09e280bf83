"""The baseline JPEG stream of the MJPG recording (loop.py:49-54,82-89), restated literally in numpy: the oracle of
tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py. A BGR u8 picture of h x w becomes SOI, a fixed
header, one interleaved 4:2:0 scan with a restart interval of one MCU row, and EOI. Integer arithmetic throughout;
the entropy coder is kept simple (a full 272 x 1024 tile takes a few seconds).

Also the case list shared by the CPU and GPU tests (cases(), case_image()) and a small marker parser (segments())."""
import hashlib

import numpy as np

# Annex K.1 / K.2, natural order
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int32)
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int32)
# ZIGZAG[k] = natural index of zig-zag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int32)

# Annex K.3 - K.6: (BITS[1..16], HUFFVAL)
DC_L = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_L = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0"
    "2433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a"
    "92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0"
    "156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a828384858687"
    "88898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HUFF = (DC_L, AC_L, DC_C, AC_C)   # the order they are written in; classes / ids 0x00, 0x10, 0x01, 0x11
HUFF_IDS = (0x00, 0x10, 0x01, 0x11)


def quant_table(base, quality):
    """The IJG quality rule on an Annex K table, natural order, int32."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base.astype(np.int64) * scale + 50) // 100, 1, 255).astype(np.int32)


def huff_codes(bits, vals):
    """symbol -> (code, length), Annex C."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """One pass of the IJG slow-integer forward DCT along the last axis of d (.., 8) int32."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    n = 11 if first else 15
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct(blocks):
    """blocks (.., 8, 8) of samples 0..255 -> coefficients scaled by 8, int32, natural order."""
    d = blocks.astype(np.int32) - 128
    d = _pass(d, True)                                    # rows
    return np.swapaxes(_pass(np.swapaxes(d, -1, -2), False), -1, -2)   # columns


def quantise(coef, qt):
    """coef (.., 8, 8) int32, qt (64,) natural -> (.., 64) int32 in zig-zag order."""
    c = coef.reshape(coef.shape[:-2] + (64,))
    d = 8 * qt
    a = (np.abs(c) + (d >> 1)) // d
    return np.where(c < 0, -a, a)[..., ZIGZAG].astype(np.int32)


def ycc(bgr):
    b, g, r = (bgr[..., i].astype(np.int32) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def downsample(c, h, w):
    """Full-resolution chroma (h, w) -> (8 ceil(h / 16), 8 ceil(w / 16)), in the order of the definition."""
    wp, mr = 16 * -(-w // 16), -(-h // 16)
    c = np.pad(c, ((0, h & 1), (0, wp - w)), mode="edge")
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = np.where(np.arange(wp // 2) & 1, 2, 1)
    s = (s + bias[None, :]) >> 2
    return np.pad(s, ((0, 8 * mr - s.shape[0]), (0, 0)), mode="edge")


def coefficients(bgr, quality):
    """Quantised zig-zag coefficients in MCU order: (MCU rows, MCUs a row, 6, 64) int32."""
    h, w = bgr.shape[:2]
    mr, mc = -(-h // 16), -(-w // 16)
    ql, qc = quant_table(K1, quality), quant_table(K2, quality)
    y, cb, cr = ycc(bgr)
    yp = np.pad(y, ((0, 16 * mr - h), (0, 16 * mc - w)), mode="edge")
    yq = quantise(fdct(_blocks(yp)), ql)                     # (2 mr, 2 mc, 64)
    out = np.zeros((mr, mc, 6, 64), np.int32)
    br, bc = -(-h // 8), -(-w // 8)
    for k in range(4):
        out[:, :, k] = yq[k >> 1::2, k & 1::2]
    for k in range(1, 4):                                    # dummy blocks: the previous block's DC, no AC
        rows = (2 * np.arange(mr) + (k >> 1)) >= br
        cols = (2 * np.arange(mc) + (k & 1)) >= bc
        dummy = rows[:, None] | cols[None, :]
        blk = out[:, :, k]
        rep = np.zeros_like(blk)
        rep[..., 0] = out[:, :, k - 1, 0]
        out[:, :, k] = np.where(dummy[..., None], rep, blk)
    out[:, :, 4] = quantise(fdct(_blocks(downsample(cb, h, w))), qc)
    out[:, :, 5] = quantise(fdct(_blocks(downsample(cr, h, w))), qc)
    return out


def _size(v):
    return int(abs(int(v))).bit_length()


class Stats:
    """What the entropy coder met (the tests assert that the case list reaches each)."""
    def __init__(self):
        self.stuffed = self.zrl = self.aligned_ends = self.unaligned_ends = 0


def scan_bytes(coef, stats=None):
    """The entropy-coded segment: every restart interval (an MCU row), RSTn between them."""
    tabs = [huff_codes(*t) for t in HUFF]
    dc_tab, ac_tab = (tabs[0], tabs[0], tabs[0], tabs[0], tabs[2], tabs[2]), (tabs[1],) * 4 + (tabs[3],) * 2
    comp = (0, 0, 0, 0, 1, 2)
    out = bytearray()
    mr, mc = coef.shape[:2]
    st = stats if stats is not None else Stats()
    for r in range(mr):
        acc, nacc = 0, 0
        pred = [0, 0, 0]

        def put(code, n):
            nonlocal acc, nacc
            acc = (acc << n) | code
            nacc += n
            while nacc >= 8:
                byte = (acc >> (nacc - 8)) & 0xFF
                nacc -= 8
                out.append(byte)
                if byte == 0xFF:
                    out.append(0)
                    st.stuffed += 1
            acc &= (1 << nacc) - 1

        for c in range(mc):
            for k in range(6):
                blk = coef[r, c, k]
                diff = int(blk[0]) - pred[comp[k]]
                pred[comp[k]] = int(blk[0])
                s = _size(diff)
                put(*dc_tab[k][s])
                if s:
                    put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
                last = 0
                for pos in np.flatnonzero(blk[1:]) + 1:
                    run = int(pos) - last - 1
                    while run > 15:
                        put(*ac_tab[k][0xF0])
                        st.zrl += 1
                        run -= 16
                    v = int(blk[pos])
                    s = _size(v)
                    put(*ac_tab[k][(run << 4) | s])
                    put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
                    last = int(pos)
                if last != 63:
                    put(*ac_tab[k][0x00])
        if nacc:
            st.unaligned_ends += 1
            put((1 << (8 - nacc)) - 1, 8 - nacc)
        else:
            st.aligned_ends += 1
        if r != mr - 1:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(out)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dqt_payloads(quality):
    return [bytes([i]) + bytes(quant_table(b, quality)[ZIGZAG].astype(np.uint8)) for i, b in enumerate((K1, K2))]


def dht_payloads():
    return [bytes([i]) + bytes(t[0]) + bytes(t[1]) for i, t in zip(HUFF_IDS, HUFF)]


def header(h, w, quality):
    """SOI .. SOS: APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS."""
    mc = -(-w // 16)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for p in dqt_payloads(quality):
        out += _seg(0xDB, p)
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") +
                bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for p in dht_payloads():
        out += _seg(0xC4, p)
    out += _seg(0xDD, mc.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(bgr, quality=75, stats=None):
    """The whole stream of a (h, w, 3) u8 BGR picture (a (h, w) grey one as B = G = R)."""
    bgr = np.asarray(bgr)
    if bgr.ndim == 2:
        bgr = np.repeat(bgr[:, :, None], 3, axis=2)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    h, w = bgr.shape[:2]
    assert 1 <= h <= 4096 and 1 <= w <= 4096
    return header(h, w, quality) + scan_bytes(coefficients(bgr, quality), stats) + b"\xff\xd9"


def segments(stream):
    """[(marker, payload)] of the header segments up to SOS, the scan bytes (after the SOS header, before EOI)."""
    assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
    i, segs = 2, []
    while True:
        assert stream[i] == 0xFF
        m = stream[i + 1]
        n = int.from_bytes(stream[i + 2:i + 4], "big")
        segs.append((m, bytes(stream[i + 4:i + 2 + n])))
        i += 2 + n
        if m == 0xDA:
            return segs, bytes(stream[i:-2])


def scan_of(stream):
    return segments(stream)[1]


def digest(scan):
    return hashlib.sha256(scan).hexdigest()[:16]


# ---- the case list (ISSUE: shapes x contents x qualities, generated from seeds) ----
SHAPES = [(1, 1), (8, 8), (17, 33), (18, 72), (24, 40), (160, 16), (40, 76), (36, 1024), (272, 1024)]
CONTENTS = ["flat", "noise", "ramp", "impulse", "checker"]
QUALITIES = [30, 75, 100]


def cases():
    """(name, h, w, content, quality): every shape with every content at the three qualities; the checkerboard at
    quality 100 only (it is there for the largest size categories)."""
    out = []
    for h, w in SHAPES:
        for content in CONTENTS:
            for q in ([100] if content == "checker" else QUALITIES):
                out.append((f"{h}x{w}-{content}-q{q}", h, w, content, q))
    return out


def case_image(h, w, content, seed=0):
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    if content == "flat":
        return np.full((h, w, 3), (40, 120, 200), np.uint8)
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(3 * xx + yy) & 255, (xx + 5 * yy) & 255, (2 * xx + 2 * yy) >> 1 & 255], axis=2).astype(np.uint8)
    if content == "impulse":
        # a flat field with a faint high-frequency pattern in every eighth block: isolated coefficients late in
        # the zig-zag order, runs of more than 15 zeros before them (ZRL)
        img = np.full((h, w, 3), 128, np.int32)
        yy, xx = np.mgrid[0:h, 0:w]
        pat = (((xx & 1) ^ (yy & 1)) * 2 - 1) * 40
        sel = ((xx // 8 + 3 * (yy // 8)) % 4 == 0)
        img += (pat * sel)[:, :, None]
        sign = rng.integers(0, 2, (h, w)) * 2 - 1
        spike = rng.random((h, w)) < 0.01
        img += (sign * spike * 60)[:, :, None]
        return np.clip(img, 0, 255).astype(np.uint8)
    if content == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    raise ValueError(content)


def avi_frames(buf):
    """The '00dc' payloads of an AVI file's movi list, in order (a minimal RIFF walk)."""
    import struct
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI "
    i, out = 12, []
    while i < len(buf):
        cc, n = struct.unpack_from("<4sI", buf, i)
        if cc == b"LIST" and buf[i + 8:i + 12] == b"movi":
            j, end = i + 12, i + 8 + n
            while j < end:
                c2, m = struct.unpack_from("<4sI", buf, j)
                assert c2 == b"00dc"
                out.append(bytes(buf[j + 8:j + 8 + m]))
                j += 8 + m + (m & 1)
        i += 8 + n + (n & 1)
    return out
