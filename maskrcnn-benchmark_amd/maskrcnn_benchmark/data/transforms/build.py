"""build_transforms (reference data/transforms/build.py): the config's INPUT section as a Compose."""
from . import transforms as T


def jitter_enabled(cfg, is_train=True):
    """does the training pipeline of this config jitter colours?  (test pipelines never do)"""
    return bool(is_train) and any(v not in (None, 0, 0.0) for v in (cfg.INPUT.BRIGHTNESS, cfg.INPUT.CONTRAST,
                                                                     cfg.INPUT.SATURATION, cfg.INPUT.HUE))


def build_transforms(cfg, is_train=True, device_prep=False):
    """device_prep: the pipeline that defers the pixels to the device: the same random draws in the same order (size,
    horizontal flip, vertical flip) and the same target, the image as a RawImage; no ToTensor / Normalize (the collator's
    RawImageBatch carries their table).  Non-zero BRIGHTNESS / CONTRAST / SATURATION / HUE are served on this path only:
    RawColorJitter draws the steps (in front of the size and flip draws, as the reference's Compose) and the batch jitters
    the raw bytes where it lands; the host pipeline keeps refusing them."""
    if is_train:
        min_size, max_size = cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN
        flip_horizontal_prob, flip_vertical_prob = cfg.INPUT.HORIZONTAL_FLIP_PROB_TRAIN, cfg.INPUT.VERTICAL_FLIP_PROB_TRAIN
        brightness, contrast = cfg.INPUT.BRIGHTNESS, cfg.INPUT.CONTRAST
        saturation, hue = cfg.INPUT.SATURATION, cfg.INPUT.HUE
    else:
        min_size, max_size = cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST
        flip_horizontal_prob = flip_vertical_prob = 0.0
        brightness = contrast = saturation = hue = 0.0
    jitter = dict(brightness=brightness, contrast=contrast, saturation=saturation, hue=hue)
    geometric = [T.Resize(min_size, max_size), T.RandomHorizontalFlip(flip_horizontal_prob),
                 T.RandomVerticalFlip(flip_vertical_prob)]
    if device_prep and jitter_enabled(cfg, is_train):
        return T.Compose([T.ToRaw(), T.RawColorJitter(**jitter)] + geometric)
    color_jitter = T.ColorJitter(**jitter)                 # the identity, or the refusal
    if device_prep:
        return T.Compose([color_jitter, T.ToRaw()] + geometric)
    normalize = T.Normalize(mean=cfg.INPUT.PIXEL_MEAN, std=cfg.INPUT.PIXEL_STD, to_bgr255=cfg.INPUT.TO_BGR255)
    return T.Compose([color_jitter] + geometric + [T.ToTensor(), normalize])
