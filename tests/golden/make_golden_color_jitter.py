"""Generate tests/golden/color_jitter_reference.npz with Pillow and numpy only (build container only; the GPU tests read
the file and never import PIL).

torchvision's ColorJitter on a PIL image is Pillow: brightness, contrast and saturation are ImageEnhance.Brightness /
Contrast / Color, hue is a uint8 add on the H plane of convert("HSV").  Those calls are made here directly.  The file
holds data only:
  image_0, image_1        [h, w, 3] uint8 sources (bytes 0 and 255, greys and every tie of the maximum among them)
  case_image [C] int32    the source of a case
  case_record [C, 8] int32  the case's jitter record (include/detops.h: four step codes, four parameters)
  expected [bytes] uint8, expected_offset [C + 1] int64: Pillow's output of case c, flat, at expected_offset[c]
Cases: every operation alone on both images at factors 0, 1, 0.6 and 1.7 (hue: shifts 0, 1, 128, 255), and all 24
orders of the four operations at fixed parameters on image_1.

Before the file is written the numpy restatement (maskrcnn_benchmark/_color_jitter_cpu.py) is compared with Pillow on
ALL 2^24 RGB colours (convert("L"), the three enhancers at seven factors, RGB -> HSV) and on all 2^24 HSV triples
(HSV -> RGB); the counts are printed (profiles/color_jitter_exhaustive.txt) and any differing byte stops the script.

Run:  python tests/golden/make_golden_color_jitter.py
"""
import importlib.util
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "_color_jitter_cpu", os.path.join(HERE, "..", "..", "maskrcnn-benchmark_amd", "maskrcnn_benchmark", "_color_jitter_cpu.py"))
J = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(J)

FACTORS = (0.0, 1.0, 0.6, 1.7)                 # 0, 1, inside (0, 1), and one that clips at both ends
SHIFTS = (0, 1, 128, 255)
EXHAUSTIVE_FACTORS = (0.0, 0.3, 0.7, 1.0, 1.4, 1.9999, 0.123456)
ORDER_PARAMS = {J.BRIGHTNESS: 1.3, J.CONTRAST: 0.7, J.SATURATION: 1.6, J.HUE: 37}
ENHANCER = {J.BRIGHTNESS: ImageEnhance.Brightness, J.CONTRAST: ImageEnhance.Contrast, J.SATURATION: ImageEnhance.Color}


def pil_hue(img, k):
    h, s, v = img.convert("HSV").split()
    h = Image.fromarray((np.asarray(h).astype(np.int64) + k).astype(np.uint8), "L")      # the uint8 add wraps
    return Image.merge("HSV", (h, s, v)).convert("RGB")


def pil_steps(rgb, steps):
    """steps: [(code, factor or k)] through Pillow"""
    img = Image.fromarray(np.ascontiguousarray(rgb), "RGB")
    for code, par in steps:
        img = pil_hue(img, par) if code == J.HUE else ENHANCER[code](img).enhance(par)
    return np.asarray(img)


def record(steps):
    rec = [0] * J.FIELDS
    for i, (code, par) in enumerate(steps):
        rec[i], rec[J.MAX_STEPS + i] = code, (int(par) if code == J.HUE else J.factor_bits(par))
    return rec


def sources():
    rng = np.random.RandomState(20245)
    a = rng.randint(0, 256, (32, 40, 3)).astype(np.uint8)
    a[0, :, :] = np.arange(40, dtype=np.uint8)[:, None] * 6                      # greys
    a[1, :20] = 0
    a[1, 20:] = 255
    a[2, :, 0] = a[2, :, 1]                                                      # ties of the maximum / minimum
    a[3, :, 1] = a[3, :, 2]
    a[4, :, 0] = a[4, :, 2]
    a[5, :, 0], a[5, :, 1] = 255, 0
    yy, xx = np.mgrid[0:29, 0:31].astype(np.float64)
    b = np.stack([255.0 * xx / 30, 255.0 * yy / 28, 127.5 + 127.5 * np.sin(0.4 * xx + 0.3 * yy)], axis=2)
    b = np.clip(np.rint(b + rng.normal(0.0, 30.0, b.shape)), 0, 255).astype(np.uint8)
    return [a, b]


def all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)


def count(name, ours, pil):
    bad = int((np.asarray(ours) != np.asarray(pil)).sum())
    print("%-34s %10d values  %d differ" % (name, np.asarray(pil).size, bad))
    assert bad == 0, name


def exhaustive():
    cube = all_colours()
    img = Image.fromarray(cube, "RGB")
    count('convert("L")', J.luma(cube), np.asarray(img.convert("L")))
    for f in EXHAUSTIVE_FACTORS:
        count("Brightness %g" % f, J.blend(0, cube, f), np.asarray(ImageEnhance.Brightness(img).enhance(f)))
        count("Color %g" % f, J.blend(J.luma(cube)[..., None], cube, f), np.asarray(ImageEnhance.Color(img).enhance(f)))
        m = J.contrast_mean(cube)
        count("Contrast %g (mean %d)" % (f, m), J.blend(m, cube, f), np.asarray(ImageEnhance.Contrast(img).enhance(f)))
    for m in (0, 1, 254, 255):                   # contrast's blend against the greys at the ends of the range
        grey = Image.new("L", img.size, m).convert("RGB")
        for f in (0.3, 1.9999):
            count("blend against grey %d at %g" % (m, f), J.blend(m, cube, f), np.asarray(Image.blend(grey, img, f)))
    count("RGB -> HSV", J.rgb_to_hsv(cube), np.asarray(img.convert("HSV")))
    count("HSV -> RGB", J.hsv_to_rgb(cube), np.asarray(Image.fromarray(cube, "HSV").convert("RGB")))


def main():
    import PIL

    print("Pillow", PIL.__version__, "numpy", np.__version__)
    exhaustive()
    images = sources()
    cases = []
    for i in range(len(images)):
        for code in (J.BRIGHTNESS, J.CONTRAST, J.SATURATION):
            cases += [(i, [(code, f)]) for f in FACTORS]
        cases += [(i, [(J.HUE, k)]) for k in SHIFTS]
    for order in itertools.permutations((J.BRIGHTNESS, J.CONTRAST, J.SATURATION, J.HUE)):
        cases.append((1, [(code, ORDER_PARAMS[code]) for code in order]))
    expected, offsets = [], [0]
    clipped_low = clipped_high = 0
    for i, steps in cases:
        want = pil_steps(images[i], steps)
        ours = J.jitter_image(images[i], record(steps))
        assert np.array_equal(ours, want), steps
        clipped_low += int((want == 0).sum())
        clipped_high += int((want == 255).sum())
        expected.append(want.reshape(-1))
        offsets.append(offsets[-1] + want.size)
    out = {"image_%d" % i: im for i, im in enumerate(images)}
    out.update({"case_image": np.asarray([i for i, _ in cases], np.int32),
                "case_record": np.asarray([record(s) for _, s in cases], np.int32),
                "expected": np.concatenate(expected), "expected_offset": np.asarray(offsets, np.int64)})
    path = os.path.join(HERE, "color_jitter_reference.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes at 0 and %d at 255 in Pillow's outputs" % (len(cases), clipped_low, clipped_high))
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
