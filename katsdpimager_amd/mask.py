"""CLEAN auto-masks: a clean mask built on the device from the residual image.

The reference has no masks; :mod:`clean` gave the minor cycle a per-pixel allow map ("CLEAN masks",
include/kimg.h), and this module builds that map the way spectral-line imagers do, per channel and
per major cycle: the pixels whose CLEAN metric stands ``sigma`` noise estimates out of the residual
(:class:`MaskThreshold`), grown by a disk of about a beam (:class:`MaskDilate`), optionally joined
with the mask of the major cycles before and cut to a user's mask.  Both steps are HIP kernels
(csrc/mask.hip); nothing comes back to the host but, on request, the pixel counts.

``Imaging.auto_mask`` strings the two together; ``frontend.process_channel(auto_mask=...)`` calls it
after every major cycle's noise estimate.
"""
import numpy as np

from . import accel
from ._lib import lib, check
from .image_plane import (ImageTemplate, border_pixels, check_polarizations, plane2d_args,
                          plane_args)
from .parameters import CLEAN_I, CLEAN_SUMSQ  # noqa: F401

#: KIMG_MASK_MAX_RADIUS
MAX_RADIUS = 64


class AutoMaskParameters:
    """``sigma``: a pixel seeds the mask where its CLEAN metric exceeds the level ``sigma`` noise
    estimates correspond to (``clean.noise_threshold_scale``, as the stopping threshold); positive.
    ``radius``: the seeds are grown by a Euclidean disk of this many pixels (0 to 64; about a beam).
    ``cumulative``: a major cycle's mask includes the masks of the major cycles before it (a source
    CLEANed below ``sigma`` stays open for the components that correct it)."""

    def __init__(self, sigma, radius, cumulative=True):
        try:
            sigma = float(sigma)
            as_int = int(radius)
        except (TypeError, ValueError):
            raise ValueError('sigma must be a number and radius an integer') from None
        if not sigma > 0:
            raise ValueError('sigma must be positive')
        if as_int != radius or not 0 <= as_int <= MAX_RADIUS:
            raise ValueError('radius must be an integer from 0 to {}'.format(MAX_RADIUS))
        self.sigma = sigma
        self.radius = as_int
        self.cumulative = bool(cumulative)

    def __repr__(self):
        return 'AutoMaskParameters({!r}, {!r}, cumulative={!r})'.format(
            self.sigma, self.radius, self.cumulative)


class MaskThreshold(accel.Operation):
    """mask = 1 where the pixel is inside the border and its CLEAN metric > threshold, else 0
    (kimg_mask_threshold).  Slots: **image** [P][H][W]; **mask** uint8 [H][W]."""

    def __init__(self, template, command_queue, image_shape, border, allocator=None):
        check_polarizations(template, image_shape)
        self.border_pixels = border_pixels(border, image_shape)
        super().__init__(command_queue, allocator)
        self.template = template
        self.slots['image'] = accel.IOSlot(image_shape, template.dtype)
        self.slots['mask'] = accel.IOSlot(image_shape[1:], np.uint8)

    def _run(self):
        pass

    def __call__(self, threshold, **kwargs):
        """``threshold`` is a metric (``clean.power_to_metric``)."""
        self.bind(**kwargs)
        self.ensure_all_bound()
        image, mask = self.buffer('image'), self.buffer('mask')
        rc = lib().kimg_mask_threshold(*plane_args(image), self.border_pixels,
                                       self.template.mode, float(threshold), *plane2d_args(mask),
                                       self.command_queue.handle)
        check(rc, 'kimg_mask_threshold')


class MaskThresholdTemplate(ImageTemplate):
    operator = MaskThreshold

    def __init__(self, context, dtype, num_polarizations, mode, tuning=None):
        super().__init__(context, dtype, num_polarizations, tuning)
        if mode not in (CLEAN_I, CLEAN_SUMSQ):
            raise ValueError('Invalid mode {}'.format(mode))
        self.mode = mode


class MaskDilate(accel.Operation):
    """dest = ((src grown by a disk) | accumulate) & restrict (kimg_mask_dilate).  Slots, all uint8
    [H][W]: **src**, **dest**, and the optional **accumulate** (may be the buffer of **dest**) and
    **restrict** (unbound = that term is dropped; ``src`` and ``restrict`` must not be ``dest``);
    **count** uint32 [counts]: entry ``index`` of a call receives the number of set pixels of
    **dest**, on the device."""

    def __init__(self, template, command_queue, shape, counts=1, allocator=None):
        super().__init__(command_queue, allocator)
        self.template = template
        self.slots['src'] = accel.IOSlot(shape, np.uint8)
        self.slots['dest'] = accel.IOSlot(shape, np.uint8)
        self.slots['accumulate'] = accel.IOSlot(shape, np.uint8, optional=True)
        self.slots['restrict'] = accel.IOSlot(shape, np.uint8, optional=True)
        self.slots['count'] = accel.IOSlot((counts,), np.uint32)

    def _run(self):
        pass

    def __call__(self, radius, index=0, **kwargs):
        self.bind(**kwargs)
        self.ensure_all_bound()
        src, dest, count = self.buffer('src'), self.buffer('dest'), self.buffer('count')
        accumulate, restrict = self.buffer('accumulate'), self.buffer('restrict')
        if not 0 <= index < count.shape[0]:
            raise ValueError('count index {} out of range'.format(index))
        H, W = src.shape
        rc = lib().kimg_mask_dilate(
            src.ptr, W, dest.ptr, W, W, H, int(radius),
            accumulate.ptr if accumulate is not None else None, W,
            restrict.ptr if restrict is not None else None, W,
            count.ptr + 4 * index, self.command_queue.handle)
        check(rc, 'kimg_mask_dilate')


class MaskDilateTemplate(ImageTemplate):
    """Masks have no dtype and no polarizations: only the context."""
    operator = MaskDilate

    def __init__(self, context, tuning=None):
        lib()
        self.context = context
