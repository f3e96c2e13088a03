"""CPU-only tests of what the cube operators share (katsdpimager_amd/cube_operator.py): the channel
pitch, the channel range and the cube shape, the twins' argument checks, the three parameter classes
that take ``channels``, the names that still import from the operators' own modules, and the
signatures of the eight operators and their templates (literals, taken from the classes before they
shared a base)."""
import ast
import glob
import inspect
import os
import types

import numpy as np
import pytest
import torch

from katsdpimager_amd import (channel_block, cube, cube_operator, cube_stats, detect, imcontsub, link,
                              smooth, sources, spectrum_stats)
from katsdpimager_amd.cube_operator import (channel_pitch, channel_range, cube_shape, host_cube,
                                            host_filled, range_in_band)

#: module, operator, parameters, and str(inspect.signature(...)) of the operator's __init__ and
#: __call__ and of its template's __init__
OPERATORS = [
    (cube, 'Moments', 'MomentParameters', '(self, template, command_queue, cube_shape)',
     '(self, cube, coordinates=None, cut=None, filled=None, channel_width=None)',
     '(self, context, params, tuning=None)'),
    (imcontsub, 'ImContSub', 'ImContSubParameters',
     "(self, template, command_queue, cube_shape, outputs=('continuum', 'rms', 'count'))",
     '(self, cube, filled=None, frequencies=None, noise=None, out=None)',
     '(self, context, params, tuning=None)'),
    (smooth, 'CubeSmooth', 'CommonBeamParameters', '(self, template, command_queue, cube_shape)',
     '(self, cube, out=None, beams=None, filled=None)', '(self, context, params)'),
    (cube_stats, 'CubeStats', 'CubeStatsParameters', '(self, template, command_queue, cube_shape)',
     '(self, cube, filled=None, region=None, update_noise=False)', '(self, context, params)'),
    (spectrum_stats, 'SpectrumStats', 'SpectrumStatsParameters',
     '(self, template, command_queue, cube_shape)', '(self, cube, filled=None, subtract=False, out=None)',
     '(self, context, params, tuning=None)'),
    (detect, 'SmoothClip', 'SmoothClipParameters', '(self, template, command_queue, cube_shape)',
     '(self, cube, filled=None, region=None)', '(self, context, params)'),
    (link, 'Link', 'LinkParameters', '(self, template, command_queue, cube_shape)',
     '(self, mask, cube, filled=None, frequencies=None)', '(self, context, params)'),
    (sources, 'Sources', 'SourceParameters', '(self, template, command_queue, cube_shape)',
     '(self, labels, cube, catalogue, filled=None, frequencies=None, tables=None)',
     '(self, context, params)'),
]

#: the three parameter classes that take ``channels``
WITH_CHANNELS = (cube.MomentParameters, cube_stats.CubeStatsParameters,
                 spectrum_stats.SpectrumStatsParameters)
BAD_RANGES = ((3, 3), (-1, 2), (0.5, 3), (True, 3), (0, 4097), 5, 'ab')


def _array(tensor):
    """What channel_pitch reads of a device array."""
    return types.SimpleNamespace(tensor=tensor, shape=tuple(tensor.shape))


def test_channel_pitch():
    shape = (3, 2, 4, 5)
    assert channel_pitch(_array(torch.zeros(shape))) == 40
    padded = torch.zeros((3, 64)).as_strided(shape, (64, 20, 5, 1))
    assert channel_pitch(_array(padded)) == 64
    # a single channel: whatever its stride says, the plane
    assert channel_pitch(_array(torch.zeros(64).as_strided((1, 2, 4, 5), (7, 20, 5, 1)))) == 40
    with pytest.raises(ValueError, match='must be dense'):
        channel_pitch(_array(torch.zeros((3, 2, 5, 4)).transpose(2, 3)))
    with pytest.raises(ValueError, match='channels overlap'):
        channel_pitch(_array(torch.zeros(200).as_strided(shape, (39, 20, 5, 1))))
    # an axis of one entry: its stride is never used
    assert channel_pitch(_array(torch.zeros(200).as_strided((3, 1, 4, 5), (20, 7, 5, 1)))) == 20
    assert channel_pitch(_array(torch.zeros(200).as_strided((3, 2, 1, 5), (10, 5, 3, 1)))) == 10
    assert channel_pitch(_array(torch.zeros(200).as_strided((3, 2, 4, 1), (8, 4, 1, 3)))) == 8


def test_channel_range_and_range_in_band():
    assert range_in_band(None, 5) == (0, 5) and range_in_band(None, 4096) == (0, 4096)
    assert channel_range((2, 5), 'channels') == (2, 5)
    assert channel_range((np.int64(2), 5.0), 'channels') == (2, 5)
    assert range_in_band(channel_range((2, 5), 'channels'), 5) == (2, 5)
    with pytest.raises(ValueError, match='beyond'):
        range_in_band(channel_range((2, 5), 'channels'), 4)
    for bad in BAD_RANGES:
        with pytest.raises(ValueError):
            channel_range(bad, 'channels')
    with pytest.raises(ValueError, match='not bools'):
        channel_range((True, 3), 'channels')
    for band in (0, 4097):
        with pytest.raises(ValueError, match='1 to 4096 channels'):
            range_in_band(None, band)


def test_cube_shape():
    assert cube_shape((1, 1, 1, 1)) == (1, 1, 1, 1)
    made = cube_shape(np.array([5, 2, 4, 3], np.int64))
    assert made == (5, 2, 4, 3) and all(type(s) is int for s in made)
    for bad in ((5, 2, 4), (5, 2, 4, 3, 1), (5, 0, 4, 3), 'abcd', None):
        with pytest.raises(ValueError, match='cube_shape must be'):
            cube_shape(bad)


def test_host_cube_and_host_filled():
    data = np.zeros((3, 2, 4), np.float32)
    assert host_cube(data) is data
    assert host_cube(np.zeros((3, 1, 2, 4), np.float32), ndim=4).shape == (3, 1, 2, 4)
    with pytest.raises(TypeError, match='cube must be float32'):
        host_cube(data.astype(np.float64))
    with pytest.raises(TypeError, match='work must be float32'):
        host_cube(data.astype(np.float64), 'work')
    with pytest.raises(ValueError):
        host_cube(np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        host_cube(data, ndim=4)
    with pytest.raises(ValueError, match='1 to 4096 channels'):
        host_cube(np.zeros((4097, 1), np.float32), band=True)
    assert host_cube(np.zeros((4097, 1), np.float32)).shape == (4097, 1)
    with pytest.raises(ValueError, match='one entry per channel'):
        host_filled([1, 1], 3)
    filled = host_filled([0, 2, 0], 3)
    assert filled.dtype == np.bool_ and filled.tolist() == [False, True, False]


@pytest.mark.parametrize('params', WITH_CHANNELS)
def test_parameter_classes_answer_alike(params):
    assert params().channels is None and params().range(5) == (0, 5)
    assert params(channels=(2, 5)).channels == (2, 5)
    assert params(channels=(2, 5)).range(5) == (2, 5)
    assert params(channels=(np.int32(0), 4096)).range(4096) == (0, 4096)
    with pytest.raises(ValueError, match='beyond'):
        params(channels=(2, 5)).range(4)
    for bad in BAD_RANGES:
        with pytest.raises(ValueError):
            params(channels=bad)
    with pytest.raises(ValueError, match='not bools'):
        params(channels=(True, 3))
    for band in (0, 4097):
        with pytest.raises(ValueError, match='1 to 4096 channels'):
            params().range(band)


def test_old_names_still_import():
    assert cube.SpectralCube is cube_operator.SpectralCube
    assert cube.MapArray is cube_operator.MapArray
    assert cube.velocities is cube_operator.velocities
    assert cube._rest_frequency is cube_operator._rest_frequency
    assert cube.SPEED_OF_LIGHT_KMS == cube_operator.SPEED_OF_LIGHT_KMS == 299792.458
    assert cube.MAX_CHANNELS == cube_operator.MAX_CHANNELS == 4096
    assert imcontsub.MAX_CHANNELS == smooth.MAX_CHANNELS == 4096
    for array in (cube.MapArray, detect.MaskCube, link.LabelCube):
        assert issubclass(array, cube_operator.ReadyArray)
        assert array.get is cube_operator.ReadyArray.get
    assert hasattr(detect.MaskCube, 'apply') and hasattr(link.LabelCube, 'mask')
    assert not hasattr(cube.Moments, '_channel_pitch')


@pytest.mark.parametrize('module,operator,params,init,call,template_init', OPERATORS,
                         ids=[row[1] for row in OPERATORS])
def test_templates_and_signatures(module, operator, params, init, call, template_init):
    op = getattr(module, operator)
    template = getattr(module, operator + 'Template')
    assert issubclass(op, cube_operator.CubeOperator)
    assert issubclass(template, channel_block.OperatorTemplate)
    assert template.operator is op and template.params_type is getattr(module, params)
    with pytest.raises(TypeError, match='params must be ' + params + '$'):
        template(None, object())
    assert str(inspect.signature(op.__init__)) == init
    assert str(inspect.signature(op.__call__)) == call
    assert str(inspect.signature(template.__init__)) == template_init
    if 'tuning' not in template_init:
        with pytest.raises(TypeError):
            template(None, object(), None)


def _bare_cube(frequencies, polarizations=(0,), channel_width=None):
    """A SpectralCube without its device array: what check_out_cube and carry_over read."""
    made = cube_operator.SpectralCube.__new__(cube_operator.SpectralCube)
    made.frequencies = np.asarray(frequencies, np.float64)
    made.polarizations = list(polarizations)
    made.channel_width = channel_width
    made.shape = (len(made.frequencies), len(made.polarizations), 2, 2)
    made.filled = np.zeros(len(made.frequencies), np.uint8)
    made.noise = np.full(len(made.frequencies), np.nan, np.float32)
    made.beams = [None] * len(made.frequencies)
    made.common_beam = None
    return made


def test_out_cube_rules():
    check = cube_operator.check_out_cube
    everything = ('shape', 'frequencies', 'polarizations', 'channel_width')
    a, b = _bare_cube([1.0, 2.0, 3.0]), _bare_cube([1.0, 2.0, 3.0])
    plain = object()
    for out in (None, a, b):
        check(a, out, 'line cube', same=everything)
    check(plain, None, 'line cube')
    check(plain, object(), 'line cube')
    with pytest.raises(TypeError, match='the line cube of a plain array is a plain array'):
        check(plain, a, 'line cube')
    with pytest.raises(TypeError, match='the line cube of a SpectralCube is a SpectralCube'):
        check(a, plain, 'line cube')
    for other, text in ((_bare_cube([1.0, 2.0, 4.0]), 'other frequencies'),
                        (_bare_cube([1.0, 2.0, 3.0], (0, 1)), 'other polarizations'),
                        (_bare_cube([1.0, 2.0, 3.0], channel_width=2.0), 'another channel width')):
        with pytest.raises(ValueError, match='out has ' + text):
            check(a, other, 'line cube', same=everything[1:])
    with pytest.raises(ValueError, match='out has another shape'):
        check(a, _bare_cube([1.0, 2.0]), 'line cube', same=everything)
    check(a, _bare_cube([1.0, 2.0, 3.0], (0, 1)), 'line cube')       # (frequencies alone by default)
    a.filled[:] = [1, 0, 1]
    a.noise[0] = 0.5
    a.beams[0] = 'beam'
    cube_operator.carry_over(a, a)
    cube_operator.carry_over(a, None)
    cube_operator.carry_over(plain, b)
    assert not b.filled.any()
    cube_operator.carry_over(a, b)
    assert b.filled.tolist() == [1, 0, 1] and b.noise[0] == np.float32(0.5) and b.beams[0] is None
    cube_operator.carry_over(a, b, beams=True)
    assert b.beams == a.beams and b.beams is not a.beams


def test_operator_filled_rules():
    op = cube_operator.CubeOperator(types.SimpleNamespace(params='p'), 'queue', (3, 1, 2, 2))
    assert (op.template.params, op.params, op.command_queue, op.cube_shape) == ('p', 'p', 'queue', (3, 1, 2, 2))
    given = [0, 2, 0]
    assert op._own_filled(object(), given, beams=None) is given
    with pytest.raises(ValueError, match='a plain array needs filled'):
        op._own_filled(object(), None)
    the_cube = _bare_cube([1.0, 2.0, 3.0])
    assert op._own_filled(the_cube, None, beams=None) is the_cube.filled
    for filled, beams in ((given, None), (None, [])):
        with pytest.raises(ValueError, match='a SpectralCube brings its own beams, filled'):
            op._own_filled(the_cube, filled, beams=beams)
    table = op._filled(given)
    assert table.dtype == np.uint8 and table.tolist() == [0, 1, 0] and table.flags.c_contiguous
    with pytest.raises(ValueError, match='one entry per channel'):
        op._filled([1, 1])
    with pytest.raises(ValueError, match='1 to 4096 channels'):
        cube_operator.CubeOperator(types.SimpleNamespace(params='p'), 'queue', (4097, 1, 2, 2), band=True)
    assert cube_operator.CubeOperator(types.SimpleNamespace(params='p'), 'queue',
                                      (4097, 1, 2, 2)).cube_shape[0] == 4097


def test_isolation():
    package = os.path.dirname(cube_operator.__file__)
    # every import statement of the shared module's text: the modules it names, the names it takes
    imported = set()
    for node in ast.walk(ast.parse(open(cube_operator.__file__).read())):
        if isinstance(node, ast.Import):
            imported.update(alias.name.split('.')[-1] for alias in node.names)
        elif isinstance(node, ast.ImportFrom):
            imported.update((node.module or '').split('.'))
            imported.update(alias.name for alias in node.names)
    assert {'accel', '_lib', 'channel_block'} <= imported
    assert not imported & {'cube', 'imcontsub', 'smooth', 'cube_stats', 'spectrum_stats', 'detect',
                           'link', 'sources'}
    for path in sorted(glob.glob(os.path.join(package, '*.py'))):
        text = open(path).read()
        assert 'Moments._channel_pitch' not in text, path
        if os.path.basename(path) != 'cube_operator.py':
            assert 'def _is_bool' not in text and 'def _device_region' not in text, path
