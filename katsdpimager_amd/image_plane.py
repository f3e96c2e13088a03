"""What the operators on dense ``[polarization][row][column]`` device images share (:mod:`.image`,
:mod:`.clean`, :mod:`.mask`, :mod:`.multiscale`, :mod:`.primary_beam`, :mod:`.weight`,
:mod:`.predict`, :mod:`.beam`): how such an array is spelled in the C ABI -- ``(ptr, row pitch,
polarization pitch, width, height, P)`` --, the shape checks and the border, the plumbing of a
template, and the two ways a call picks its entry point (by precision, by mask).  The counterpart
of :mod:`.channel_block` for the image plane; it imports none of the operators.
"""
import numpy as np

from . import types
from ._lib import lib, check


# ---- a dense array as the library's arguments ----------------------------------------------------
def plane_pitches(array):
    """``(row pitch, polarization pitch)`` of a dense [P][H][W] array, in elements."""
    return array.shape[2], array.shape[1] * array.shape[2]


def plane_args(array):
    """``(ptr, row pitch, polarization pitch, width, height, P)`` of a dense [P][H][W] array."""
    P, H, W = array.shape
    return array.ptr, W, H * W, W, H, P


def psf_args(psf):
    """``(ptr, row pitch, polarization pitch, width, height)``: a PSF beside an image, whose P it
    shares."""
    return plane_args(psf)[:5]


def plane2d_args(array):
    """``(ptr, row pitch)`` of a dense [H][W] array (a mask, a beam plane)."""
    return array.ptr, array.shape[1]


def pol_ptr(array, pol):
    """Device address of polarization `pol` of a [P][H][W] array."""
    return array.ptr + pol * array.shape[1] * array.shape[2] * array.dtype.itemsize


# ---- shapes --------------------------------------------------------------------------------------
def border_pixels(border, shape, checked=True):
    """The border of a [P][H][W] image in pixels: ``border`` is a fraction of the smaller side.
    ``checked=False`` for the one caller that takes any border (the numpy twin of multi-scale
    CLEAN)."""
    if checked and border >= 0.5:
        raise ValueError('Border must be less than half the image size')
    return round(border * min(shape[1], shape[2]))


def check_polarizations(template, *shapes):
    for shape in shapes:
        if shape[0] != template.num_polarizations:
            raise ValueError('Mismatch in number of polarizations')


def check_image_shape(template, shape):
    if len(shape) != 3:
        raise ValueError('Wrong number of dimensions in shape')
    check_polarizations(template, shape)


# ---- templates -----------------------------------------------------------------------------------
class ImageTemplate:
    """``Template(context, dtype, num_polarizations).instantiate(command_queue, ...)`` makes
    :attr:`operator`.  A template that takes something else keeps an ``__init__`` of its own."""

    operator = None
    #: whether float64 is taken beside float32 (the ``kimg_*_f64`` calls)
    float64 = False

    def __init__(self, context, dtype, num_polarizations, tuning=None):
        require = types.require_float32_or_64 if self.float64 else types.require_float32
        require(dtype, type(self).__name__)
        lib()
        self.context = context
        self.dtype = np.dtype(dtype)
        self.num_polarizations = num_polarizations

    def instantiate(self, *args, **kwargs):
        return self.operator(self, *args, **kwargs)


# ---- which entry point ---------------------------------------------------------------------------
#: the calls with a ``_f64`` twin that takes the same arguments
PRECISION_PAIRS = ('kimg_grid_to_layer', 'kimg_layer_to_grid', 'kimg_layer_to_image',
                   'kimg_image_to_layer', 'kimg_scale', 'kimg_add_image', 'kimg_apply_primary_beam')


def precision_call(name, dtype):
    """``(function, its name)``: ``name`` for float32 images, ``name + '_f64'`` for float64."""
    if name not in PRECISION_PAIRS:
        raise ValueError('{} has no float64 form'.format(name))
    types.require_float32_or_64(dtype, name)
    if np.dtype(dtype) == np.float64:
        name += '_f64'
    return getattr(lib(), name), name


def masked_call(name, mask, queue, *args):
    """``name(*args)``, or with a CLEAN mask (uint8 [H][W]) ``name + '_masked'`` with
    ``(mask, its row pitch)`` appended (include/kimg.h, "CLEAN masks")."""
    if mask is not None:
        mask.used_on(queue)
        name += '_masked'
        args += plane2d_args(mask)
    check(getattr(lib(), name)(*args), name)
