"""What the operators on a spectral cube share (:mod:`.cube`'s moments, :mod:`.imcontsub`,
:mod:`.smooth`, :mod:`.cube_stats`, :mod:`.spectrum_stats`, :mod:`.detect`, :mod:`.link`,
:mod:`.sources`; the device side is csrc/kimg_cube_column.h and csrc/kimg_cube_labels.h): the
container :class:`SpectralCube`, the result arrays that carry a ``ready`` event, the checks of a cube
shape, a channel range, an input array, ``filled`` and an ``out=`` cube, and the plumbing of a device
operator.  The numpy twins, every operator's arithmetic and its tables stay in their own modules; this
module imports none of them.
"""
import numpy as np

from . import accel
from ._lib import lib, check
from .channel_block import integer, OperatorTemplate

#: KIMG_MOMENTS_MAX_CHANNELS
MAX_CHANNELS = 4096
#: km/s
SPEED_OF_LIGHT_KMS = 299792.458
#: the spectral axes a cube's coordinates come in
AXES = ('velocity', 'frequency')


# ---- small checks --------------------------------------------------------------------------------
def is_bool(value):
    return isinstance(value, (bool, np.bool_))


def band_size(num_channels):
    """``num_channels`` as an int, 1 to :data:`MAX_CHANNELS`."""
    num_channels = int(num_channels)
    if not 1 <= num_channels <= MAX_CHANNELS:
        raise ValueError('1 to {} channels'.format(MAX_CHANNELS))
    return num_channels


def channel_range(pair, what):
    """``pair`` = (first, stop) as two ints, ``0 <= first < stop <= MAX_CHANNELS``; bools are
    refused."""
    try:
        first, stop = pair
    except (TypeError, ValueError):
        raise ValueError('{} must be (first, stop)'.format(what)) from None
    if is_bool(first) or is_bool(stop):
        raise ValueError('{} must be integers, not bools'.format(what))
    first = integer(first, 'the first channel of ' + what, 0, MAX_CHANNELS - 1)
    stop = integer(stop, 'the stop channel of ' + what, first + 1, MAX_CHANNELS)
    return first, stop


def range_in_band(channels, num_channels):
    """(first, stop) of ``channels`` (a :func:`channel_range`, or None: all) within a band of
    ``num_channels`` channels."""
    num_channels = band_size(num_channels)
    if channels is None:
        return 0, num_channels
    if channels[1] > num_channels:
        raise ValueError('channels {} beyond the {} of the cube'.format(channels, num_channels))
    return channels


def cube_shape(shape):
    """``shape`` as the tuple (C, P, H, W) of ints, each 1 or more."""
    try:
        shape = tuple(int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError('cube_shape must be (C, P, H, W)') from None
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError('cube_shape must be (C, P, H, W)')
    return shape


_checked_shape = cube_shape         # (for where ``cube_shape`` is an argument's name)


def channel_pitch(array):
    """Elements from one channel of a [C][P][H][W] device array to the next.  The [P][H][W] plane
    must be dense; the channel axis may have any pitch that keeps channels apart (a view of a larger
    tensor)."""
    C, P, H, W = array.shape
    strides = array.tensor.stride()
    if (W > 1 and strides[3] != 1) or (H > 1 and strides[2] != W) or (P > 1 and strides[1] != H * W):
        raise ValueError('the [polarization][m][l] plane must be dense')
    if C == 1:
        return P * H * W
    if strides[0] < P * H * W:
        raise ValueError('channels overlap')
    return int(strides[0])


# ---- the numpy twins' argument checks ------------------------------------------------------------
def host_cube(cube, what='cube', ndim=None, band=False):
    """``cube`` as a float32 host array [channel][...plane], or with ``ndim=4``
    [channel][polarization][y][x]; ``band``: of 1 to :data:`MAX_CHANNELS` channels."""
    cube = np.asarray(cube)
    if cube.dtype != np.float32:
        raise TypeError('{} must be float32'.format(what))
    if ndim is None and cube.ndim < 2:
        raise ValueError('{} must be [channel][...plane]'.format(what))
    if ndim == 4 and cube.ndim != 4:
        raise ValueError('{} must be [channel][polarization][y][x]'.format(what))
    if band:
        band_size(cube.shape[0])
    return cube


def host_filled(filled, num_channels):
    """``filled`` as a bool array [C]: any nonzero entry reads as filled."""
    filled = np.asarray(filled) != 0
    if filled.shape != (num_channels,):
        raise ValueError('filled must have one entry per channel')
    return filled


def host_plane_mask(mask, shape, what):
    """``mask`` (uint8 or bool, of ``shape``) as a bool array."""
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 and mask.dtype != np.bool_:
        raise TypeError('{} must be uint8 or bool'.format(what))
    if mask.shape != tuple(shape):
        raise ValueError('{} of shape {} where {} is needed'.format(what, mask.shape, tuple(shape)))
    return mask != 0


# ---- the container -------------------------------------------------------------------------------
def _rest_frequency(value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError('rest_frequency must be a number') from None
    if not 0.0 < value < np.inf:                    # (false for NaN)
        raise ValueError('rest_frequency must be finite and above 0')
    return value


def velocities(frequencies, rest_frequency):
    """The radio convention ``c (1 - f / f0)`` in km/s, float64."""
    f0 = _rest_frequency(rest_frequency)
    return (1.0 - np.asarray(frequencies, np.float64) / f0) * SPEED_OF_LIGHT_KMS


class SpectralCube:
    """The images of ``len(frequencies)`` channels in ONE device allocation, float32
    [channel][polarization][m][l], NaN until a plane is :meth:`put`.

    ``frequencies``: float64 [C], Hz, strictly monotonic (ValueError otherwise).  ``polarizations``:
    the list of polarization ids of every plane (``image_parameters.fixed.polarizations``), or their
    number.  ``shape`` = (height, width) of a plane.  ``channel_width`` (Hz): needed only for moments
    over a single channel.

    All planes share one pixel size and one image centre; that is the caller's business -- the
    reference chooses a pixel size per band, which is what a cube needs.  Every plane keeps its own
    restoring beam: ``beams`` (a list, one entry per channel) holds what :meth:`put` was told of it,
    None where nothing; ``common_beam`` is None until ``smooth.CubeSmooth`` has made a cube whose
    planes share one, and is then that beam.

    ``array`` is the device array, ``filled`` (uint8 [C]) says which planes hold an image and ``noise``
    (float32 [C], NaN = none) what :meth:`put` was told of them."""

    def __init__(self, context, queue, frequencies, polarizations, shape, channel_width=None):
        frequencies = np.array(frequencies, np.float64)
        if frequencies.ndim != 1 or not 1 <= len(frequencies) <= MAX_CHANNELS:
            raise ValueError('frequencies must be [channel], 1 to {} of them'.format(MAX_CHANNELS))
        if not np.all(np.isfinite(frequencies)):
            raise ValueError('frequencies must be finite')
        steps = np.diff(frequencies)
        if len(steps) and not (np.all(steps > 0) or np.all(steps < 0)):
            raise ValueError('frequencies must be strictly monotonic')
        if isinstance(polarizations, (int, np.integer)):
            polarizations = list(range(int(polarizations)))
        self.polarizations = list(polarizations)
        try:
            height, width = (int(s) for s in shape)
        except (TypeError, ValueError):
            raise ValueError('shape must be (height, width)') from None
        if not self.polarizations or height < 1 or width < 1:
            raise ValueError('an empty plane')
        if channel_width is not None:
            channel_width = float(channel_width)
            if channel_width != channel_width or channel_width == 0.0:
                raise ValueError('channel_width must be a number other than 0')
        self.context = context
        self.command_queue = queue
        self.frequencies = frequencies
        self.channel_width = channel_width
        C = len(frequencies)
        self.shape = (C, len(self.polarizations), height, width)
        self.filled = np.zeros(C, np.uint8)
        self.noise = np.full(C, np.nan, np.float32)
        self.beams = [None] * C
        self.common_beam = None
        self.array = accel.DeviceArray(context, self.shape, np.float32, queue=queue)
        check(lib().kimg_fill(self.array.ptr, int(np.prod(self.shape)), float('nan'), queue.handle),
              'kimg_fill')

    @classmethod
    def like(cls, cube, queue):
        """A new, empty cube on ``queue`` with the frequencies, polarizations, plane and channel
        width of ``cube``."""
        return cls(queue.context, queue, cube.frequencies, cube.polarizations, cube.shape[2:],
                   cube.channel_width)

    def put(self, channel, image, noise=None, wait_for=None, beam=None):
        """Copy ``image`` -- a device array [P][H][W] (an imager's buffer will do) or a host array --
        into plane ``channel``, on the cube's queue, and record the channel's ``noise``
        (``result['noise']`` of ``process_channel``) and restoring ``beam`` (a ``beam.Beam`` in
        pixels, as ``beam.fit_beam`` returns it; ``smooth.CubeSmooth`` needs one for every plane).

        The copy is ordered after the cube queue's own work only.  An image that another queue is
        still writing needs ``wait_for``: events of that queue (``queue.enqueue_marker()``), which the
        cube's queue waits for on the device before it copies.  ``process_channel`` itself waits for
        the imager before it returns; what is enqueued after it (``add_model_to_dirty``) does not.
        Returns an event of the cube's queue that fires when the copy is done: the image's queue
        waits for it (``enqueue_wait_for_events``) before it writes the buffer again."""
        try:
            as_int = int(channel)
        except (TypeError, ValueError):
            raise TypeError('channel must be an integer') from None
        if as_int != channel or not 0 <= as_int < self.shape[0]:
            raise ValueError('no channel {!r} in a cube of {}'.format(channel, self.shape[0]))
        device = isinstance(image, accel.DeviceArray)
        if not device:
            image = np.asarray(image)
        if image.dtype != np.float32:
            raise TypeError('image must be float32, not {}'.format(image.dtype))
        if tuple(image.shape) != self.shape[1:]:
            raise ValueError('image of shape {} for planes of {}'.format(tuple(image.shape), self.shape[1:]))
        if noise is not None:
            noise = np.float32(noise)
        queue = self.command_queue
        if wait_for:
            queue.enqueue_wait_for_events(wait_for)
        if device:
            image.copy_region(queue, self.array, np.s_[:], np.s_[as_int])
        else:
            self.array.set_region(queue, image, np.s_[as_int], np.s_[:])
        self.filled[as_int] = 1
        self.noise[as_int] = np.nan if noise is None else noise
        self.beams[as_int] = beam
        return queue.enqueue_marker()

    def get(self, queue=None):
        """The cube as a host array (waits for the queue)."""
        return self.array.get(self.command_queue if queue is None else queue)

    def coordinates(self, axis='frequency', rest_frequency=None):
        """float64 [C]: the frequencies (Hz), or with 'velocity' the radio velocities
        ``c (1 - f / rest_frequency)`` in km/s."""
        if axis == 'frequency':
            return self.frequencies.copy()
        if axis == 'velocity':
            if rest_frequency is None:
                raise ValueError('the velocity axis needs a rest frequency')
            return velocities(self.frequencies, rest_frequency)
        raise ValueError("axis must be 'velocity' or 'frequency'")

    def axis_channel_width(self, axis='frequency', rest_frequency=None):
        """``channel_width`` on the axis (Hz or km/s, absolute), or None."""
        if self.channel_width is None:
            return None
        if axis == 'frequency':
            return abs(self.channel_width)
        return abs(self.channel_width) / _rest_frequency(rest_frequency) * SPEED_OF_LIGHT_KMS


# ---- result arrays -------------------------------------------------------------------------------
def wait_ready(queue, array):
    """Make ``queue`` wait on the device for ``array.ready``, where the array has one."""
    ready = getattr(array, 'ready', None)
    if ready is not None:
        queue.enqueue_wait_for_events([ready])


def mark_ready(queue, arrays):
    """One marker of ``queue`` as the ``ready`` of every one of ``arrays``."""
    ready = queue.enqueue_marker()
    for array in arrays:
        array.ready = ready
    return ready


class ReadyArray(accel.DeviceArray):
    """A device array that an operator's call returns.  ``ready`` fires when the call has written it,
    and :meth:`get` makes its queue wait for that on the device first, so a read on ANY queue sees
    the finished array; kernels of other queues that take the raw pointer wait for ``ready``
    themselves (``queue.enqueue_wait_for_events([array.ready])``).  Arrays of a whole cube also say
    which ``filled`` (uint8 [C]) their call was told and on which ``command_queue`` it ran."""

    ready = None
    filled = None
    command_queue = None

    @classmethod
    def of_cube(cls, queue, shape, dtype, filled):
        """A new array [C][P][H][W] for a call on ``queue`` that was told ``filled``."""
        array = cls(queue.context, shape, dtype, queue=queue)
        array.command_queue = queue
        array.filled = filled.copy()
        return array

    def get(self, command_queue, ary=None):
        wait_ready(command_queue, self)
        return super().get(command_queue, ary)


class MapArray(ReadyArray):
    """A map [P][H][W] of one call of :class:`cube.Moments`, :class:`imcontsub.ImContSub` or
    :class:`spectrum_stats.SpectrumStats`."""


# ---- out= cubes ----------------------------------------------------------------------------------
_OTHER = {'shape': 'another shape', 'frequencies': 'other frequencies',
          'polarizations': 'other polarizations', 'channel_width': 'another channel width'}


def check_out_cube(cube, out, what, same=('frequencies',)):
    """The rules of an ``out=`` that is neither None nor ``cube`` itself: it is a
    :class:`SpectralCube` if and only if ``cube`` is one (TypeError, which names the result as
    ``what``), and then equals it in every attribute of ``same`` (ValueError)."""
    if out is None or out is cube:
        return
    if not isinstance(cube, SpectralCube):
        if isinstance(out, SpectralCube):
            raise TypeError('the {} of a plain array is a plain array'.format(what))
        return
    if not isinstance(out, SpectralCube):
        raise TypeError('the {} of a SpectralCube is a SpectralCube'.format(what))
    for name in same:
        if not np.array_equal(getattr(out, name), getattr(cube, name)):
            raise ValueError('out has ' + _OTHER[name])


def carry_over(cube, out, beams=False):
    """After a call has written the SpectralCube ``out`` from another, ``cube``: ``filled`` and
    ``noise`` go with the planes, and with ``beams`` the beams too."""
    if not isinstance(cube, SpectralCube) or out is None or out is cube:
        return
    out.filled[:] = cube.filled
    out.noise[:] = cube.noise
    if beams:
        out.beams = list(cube.beams)
        out.common_beam = cube.common_beam


def blank_stale_planes(queue, out_array, out_pitch, stale_channels, plane_elements):
    """NaN into the planes ``stale_channels`` of ``out_array``: those an ``out=`` cube had filled
    and its source has not, back to what an unfilled plane holds."""
    for c in stale_channels:
        check(lib().kimg_fill(out_array.ptr + 4 * int(c) * out_pitch, plane_elements, float('nan'),
                              queue.handle), 'kimg_fill')


# ---- the device operators ------------------------------------------------------------------------
class CubeOperator:
    """What an operator made for cubes of ``cube_shape`` = (C, P, H, W) on ``command_queue`` keeps,
    and the checks of what it is called with.  ``band``: C above :data:`MAX_CHANNELS` is refused here,
    for the operators whose parameters do not refuse it themselves."""

    _region = None

    def __init__(self, template, command_queue, cube_shape, band=False):
        self.template = template
        self.params = template.params
        self.command_queue = command_queue
        self.cube_shape = _checked_shape(cube_shape)
        if band:
            band_size(self.cube_shape[0])

    def _arrays(self, *items):
        """The device arrays of ``(obj, what, dtype)`` items, each a :class:`SpectralCube` or an
        :class:`accel.DeviceArray` of that dtype and the operator's shape; every item's TypeError
        comes before any shape's ValueError."""
        arrays = []
        for obj, what, dtype in items:
            array = obj.array if isinstance(obj, SpectralCube) else obj
            if not isinstance(array, accel.DeviceArray):
                raise TypeError('{} must be a SpectralCube or a DeviceArray'.format(what))
            if array.dtype != dtype:
                raise TypeError('{} must be {}'.format(what, np.dtype(dtype).name))
            arrays.append(array)
        for array in arrays:
            if tuple(array.shape) != self.cube_shape:
                raise ValueError('the operator was made for cubes of {}, this one is {}'.format(
                    self.cube_shape, tuple(array.shape)))
        return arrays

    def _array(self, obj, what, dtype=np.float32):
        return self._arrays((obj, what, dtype))[0]

    def _own_filled(self, cube, filled, **brings):
        """The ``filled`` of a call, as it was given: a :class:`SpectralCube` brings its own, and
        whatever else it brings (``brings``: those arguments by name) must then be None too; a plain
        array needs one."""
        if isinstance(cube, SpectralCube):
            if filled is not None or any(value is not None for value in brings.values()):
                raise ValueError('a SpectralCube brings its own ' + ', '.join(list(brings) + ['filled']))
            return cube.filled
        if filled is None:
            raise ValueError('a plain array needs filled')
        return filled

    def _filled(self, filled):
        """``filled`` as the host uint8 [C] table the entry points take."""
        return host_filled(filled, self.cube_shape[0]).view(np.uint8)

    def _wait_ready(self, array):
        wait_ready(self.command_queue, array)

    def _device_region(self, region):
        """``region`` (uint8 or bool [H][W]) on the device: a dense device array as it is, a host
        array uploaded into the operator's own."""
        queue = self.command_queue
        H, W = self.cube_shape[2:]
        if isinstance(region, accel.DeviceArray):
            if region.dtype != np.uint8 and region.dtype != np.bool_:
                raise TypeError('region must be uint8 or bool')
            if tuple(region.shape) != (H, W):
                raise ValueError('region of shape {} for planes of {}'.format(tuple(region.shape), (H, W)))
            if W > 1 and region.tensor.stride()[1] != 1 or H > 1 and region.tensor.stride()[0] != W:
                raise ValueError('region must be dense')
            region.used_on(queue)
            return region
        host = host_plane_mask(region, (H, W), 'region').view(np.uint8)
        if self._region is None:
            self._region = accel.DeviceArray(queue.context, (H, W), np.uint8, queue=queue)
        self._region.set(queue, host)
        return self._region


class CubeTemplate(OperatorTemplate):
    """An :class:`channel_block.OperatorTemplate` that takes no ``tuning``."""

    def __init__(self, context, params):
        super().__init__(context, params)
