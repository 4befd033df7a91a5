"""Host implementation of the colour jitter defined in include/detops.h (detops_color_jitter_u8), for CPU tensors
(numpy): Pillow's ImageEnhance.Brightness / Contrast / Color (Image.blend against a degenerate image), convert("L") and
the round trip through convert("HSV"), restated on arrays.  numpy's float32 and float64 operations are single IEEE
operations (nothing is contracted), which is what the definition asks for.

A jitter record is int32 [8] per image: four step codes in the order they run (0 ends the list) and, at the same index
+ 4, the step's parameter: the fp32 bits of the factor (brightness, contrast, saturation) or the byte shift k (hue).
"""
import numpy as np

NONE, BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3, 4
FIELDS = 8                     # int32 per image: 4 step codes, 4 parameters
MAX_STEPS = 4


def luma(rgb):
    """L of Pillow's convert("L"): rgb [..., 3] uint8 -> int64 [...]"""
    p = rgb.astype(np.int64)
    return (p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16


def blend(d, x, factor):
    """Image.blend(degenerate, image, factor) per byte: d, x integer arrays (broadcast) -> uint8"""
    a = np.float32(factor)
    d = np.asarray(d, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    t = d.astype(np.float32) + a * (x - d).astype(np.float32)
    if np.float32(0) <= a <= np.float32(1):
        return np.trunc(t).astype(np.uint8)
    return np.trunc(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8)


def contrast_mean(rgb):
    """the grey level contrast blends against: int(S / (h * w) + 0.5) in fp64, S the integer sum of L over the image"""
    lum = luma(rgb)
    return int(float(int(lum.sum())) / float(lum.size) + 0.5)


def rgb_to_hsv(rgb):
    """Pillow's convert("HSV") of rgb [..., 3] uint8 -> uint8 [..., 3]"""
    p = rgb.astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    maxc, minc = p.max(axis=-1), p.min(axis=-1)
    grey = maxc == minc
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc = (maxc - r).astype(f32) / cr
        gc = (maxc - g).astype(f32) / cr
        bc = (maxc - b).astype(f32) / cr
        h_r = bc - gc
        h_g = ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(f32)
        h_b = ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(f32)
        h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
        hh = np.clip(np.trunc(np.where(grey, 0.0, h.astype(np.float64) * 255.0)), 0, 255)
        ss = np.clip(np.trunc(np.where(grey, 0.0, s.astype(np.float64) * 255.0)), 0, 255)
    return np.stack([hh.astype(np.uint8), ss.astype(np.uint8), maxc.astype(np.uint8)], axis=-1)


def _round8(x):
    """round half away from zero of x >= 0 (fp64), clipped to a byte"""
    r = np.floor(x)
    r = r + ((x - r) >= 0.5)
    return np.clip(r, 0, 255).astype(np.uint8)


def hsv_to_rgb(hsv):
    """Pillow's HSV -> RGB conversion of hsv [..., 3] uint8 -> uint8 [..., 3]"""
    H, S, V = (hsv[..., c].astype(np.float64) for c in range(3))
    h6 = H * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    fs = (S / 255.0).astype(np.float32).astype(np.float64)
    p = _round8(V * (1.0 - fs))
    q = _round8(V * (1.0 - fs * f))
    t = _round8(V * (1.0 - fs * (1.0 - f)))
    v = hsv[..., 2]
    case = i.astype(np.int64) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.empty(hsv.shape, dtype=np.uint8)
    for c in range(3):
        out[..., c] = np.choose(case, [row[c] for row in table])
    grey = hsv[..., 1] == 0
    out[grey] = v[grey][..., None]
    return out


def hue_shift(rgb, k):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(k)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def factor_bits(f):
    """the parameter field of a brightness / contrast / saturation step: the fp32 bits of the factor"""
    return int(np.array([f], dtype=np.float32).view(np.int32)[0])


def bits_factor(bits):
    return np.array([bits], dtype=np.int32).view(np.float32)[0]


def check_records(jitter):
    """the refusals of the entry point: an unknown code, a code after the list's end, an operation twice, k outside
    0 .. 255, a non-finite factor"""
    jitter = np.asarray(jitter)
    for rec in jitter.reshape(-1, FIELDS).tolist():
        seen, ended = set(), False
        for code, par in zip(rec[:MAX_STEPS], rec[MAX_STEPS:]):
            if code == NONE:
                ended = True
                continue
            if code not in (BRIGHTNESS, CONTRAST, SATURATION, HUE):
                raise ValueError("color_jitter: unknown step code %d" % code)
            if ended:
                raise ValueError("color_jitter: step %d after the end of the list" % code)
            if code in seen:
                raise ValueError("color_jitter: step %d given twice" % code)
            seen.add(code)
            if code == HUE:
                if not 0 <= par <= 255:
                    raise ValueError("color_jitter: hue shift %d outside 0 .. 255" % par)
            elif not np.isfinite(bits_factor(par)):
                raise ValueError("color_jitter: non-finite factor")


def steps_of(record):
    """[(code, parameter field)] of one record, in order"""
    rec = [int(v) for v in record]
    out = []
    for code, par in zip(rec[:MAX_STEPS], rec[MAX_STEPS:]):
        if code == NONE:
            break
        out.append((code, par))
    return out


def jitter_image(rgb, record):
    """rgb [h, w, 3] uint8 -> a new array: the record's steps in order"""
    out = np.array(rgb, dtype=np.uint8)
    for code, par in steps_of(record):
        if code == BRIGHTNESS:
            out = blend(0, out, bits_factor(par))
        elif code == CONTRAST:
            out = blend(contrast_mean(out), out, bits_factor(par))
        elif code == SATURATION:
            out = blend(luma(out)[..., None], out, bits_factor(par))
        elif code == HUE:
            out = hue_shift(out, par)
        else:
            raise ValueError("color_jitter: unknown step code %d" % code)
    return out


def color_jitter(raw, offsets, geom, jitter):
    """IN PLACE on raw [bytes] uint8: image i = raw[offsets[i] : offsets[i] + 3 h w], (h, w) = geom[i, :2]"""
    check_records(jitter)
    for off, g in zip(offsets.tolist(), geom.tolist()):            # everything is validated before a byte changes
        if g[0] < 1 or g[1] < 1 or off < 0 or off + 3 * g[0] * g[1] > raw.shape[0]:
            raise ValueError("color_jitter: an image outside the buffer")
    for off, g, rec in zip(offsets.tolist(), geom.tolist(), jitter.tolist()):
        h, w = int(g[0]), int(g[1])
        if rec[0] == NONE:
            continue
        raw[off:off + 3 * h * w] = jitter_image(raw[off:off + 3 * h * w].reshape(h, w, 3), rec).reshape(-1)
    return raw
