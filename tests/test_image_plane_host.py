"""What the image-plane operators share (katsdpimager_amd/image_plane.py) and what must not have
moved when they were put on it: the argument spelling, every template's attributes and error texts,
the border, the masked and the float64 calls, the route of the grid <-> image operations, and the
return codes of csrc/image.hip.  CPU only but for the last test; the expectations are literals,
those about the operators and the library taken from the code before it shared anything."""
import ctypes
import itertools
import types

import numpy as np
import pytest

from katsdpimager_amd import (_lib, accel, beam, clean, image, image_plane, mask, multiscale,
                              parameters, predict, primary_beam, weight)

EINVAL, EUNSUPPORTED = -10001, -10002


class FakeArray:
    """A device array as the helpers see one: ``ptr``, ``shape``, ``dtype``."""
    def __init__(self, ptr, shape, dtype):
        self.ptr, self.shape, self.dtype = ptr, tuple(shape), np.dtype(dtype)
        self.used = []
        n = int(np.prod(shape))
        self.tensor = types.SimpleNamespace(numel=lambda: n,
                                            element_size=lambda: self.dtype.itemsize)

    def used_on(self, queue):
        self.used.append(queue)


CONTEXT = object()
QUEUE = types.SimpleNamespace(context=CONTEXT, handle=0x5000)


# ---- the argument spelling -------------------------------------------------------------------
def test_plane_arguments():
    a = FakeArray(0x1000, (3, 5, 7), np.float32)
    b = FakeArray(0x2000, (2, 4, 6), np.float64)
    assert image_plane.plane_args(a) == (0x1000, 7, 35, 7, 5, 3)
    assert image_plane.plane_args(b) == (0x2000, 6, 24, 6, 4, 2)
    assert image_plane.plane_pitches(a) == (7, 35)
    assert image_plane.plane_pitches(b) == (6, 24)
    assert image_plane.psf_args(a) == (0x1000, 7, 35, 7, 5)
    assert image_plane.psf_args(b) == (0x2000, 6, 24, 6, 4)
    # polarization 2 of a: 2 planes of 5 * 7 float32 = 280 bytes on; 1 of b: 4 * 6 float64 = 192
    assert image_plane.pol_ptr(a, 0) == 0x1000
    assert image_plane.pol_ptr(a, 2) == 0x1000 + 280
    assert image_plane.pol_ptr(b, 1) == 0x2000 + 192
    assert image_plane.plane2d_args(FakeArray(0x3000, (5, 7), np.uint8)) == (0x3000, 7)


BORDERS = [
    ((1, 64, 64), (0, 16, 31)),
    ((4, 33, 70), (0, 8, 16)),
    ((2, 70, 33), (0, 8, 16)),
]


@pytest.mark.parametrize('shape, expected', BORDERS)
def test_border_pixels(shape, expected):
    for border, pixels in zip((0.0, 0.25, 0.49), expected):
        assert image_plane.border_pixels(border, shape) == pixels
        # ... and the callers that keep it
        noise = clean.NoiseEstTemplate(CONTEXT, np.float32, shape[0]).instantiate(QUEUE, shape, border)
        assert noise.border_pixels == pixels
        seeds = mask.MaskThresholdTemplate(CONTEXT, np.float32, shape[0], parameters.CLEAN_I)
        assert seeds.instantiate(QUEUE, shape, border).border_pixels == pixels
    assert image_plane.border_pixels(0.25, (1, 34, 34)) == 8         # 8.5: round half to even
    assert image_plane.border_pixels(0.75, (1, 64, 64), checked=False) == 48
    with pytest.raises(ValueError, match='^Border must be less than half the image size$'):
        image_plane.border_pixels(0.5, (1, 64, 64))


def test_shape_checks():
    template = types.SimpleNamespace(num_polarizations=2)
    image_plane.check_polarizations(template, (2, 8, 8), (2, 4, 4))
    image_plane.check_image_shape(template, (2, 8, 8))
    with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
        image_plane.check_polarizations(template, (2, 8, 8), (3, 8, 8))
    with pytest.raises(ValueError, match='^Wrong number of dimensions in shape$'):
        image_plane.check_image_shape(template, (2, 8))
    with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
        image_plane.check_image_shape(template, (1, 8, 8))


# ---- the templates ---------------------------------------------------------------------------
def _clean_parameters(border=0.25, mode=parameters.CLEAN_I):
    return parameters.CleanParameters(100, 0.1, 0.85, 5.0, mode, 0.01, 0.5, border)


def _image_parameters(pols, pixels=64, dtype=np.float32):
    fixed = parameters.FixedImageParameters(list(range(pols)), dtype)
    return parameters.ImageParameters(fixed, 1.0, None, 0.2, None, pixel_size=1e-5, pixels=pixels)


SCALES = multiscale.MultiScaleParameters([0, 4])

#: name: (how it is made from (dtype, P), the operator it makes, float64 allowed, the name of its
#: dtype attribute, arguments of instantiate after the queue for a [2][16][16] image)
TEMPLATES = {
    'ScaleTemplate': (lambda d, P: image.ScaleTemplate(CONTEXT, d, P), image.Scale, True, 'dtype',
                      ((2, 16, 16),)),
    'AddImageTemplate': (lambda d, P: image.AddImageTemplate(CONTEXT, d, P), image.AddImage, True,
                         'dtype', ((2, 16, 16),)),
    'ApplyPrimaryBeamTemplate': (lambda d, P: image.ApplyPrimaryBeamTemplate(CONTEXT, d, P),
                                 image.ApplyPrimaryBeam, True, 'dtype', ((2, 16, 16), 0.1, 0.0)),
    'LayerToImageTemplate': (lambda d, P: image.LayerToImageTemplate(CONTEXT, d), image.LayerToImage,
                             True, 'real_dtype', ((2, 16, 16), 1e-3, -8e-3)),
    'ImageToLayerTemplate': (lambda d, P: image.ImageToLayerTemplate(CONTEXT, d), image.ImageToLayer,
                             True, 'real_dtype', ((2, 16, 16), 1e-3, -8e-3)),
    'PsfPatchTemplate': (lambda d, P: clean.PsfPatchTemplate(CONTEXT, d, P), clean.PsfPatch, False,
                         'dtype', ((2, 16, 16),)),
    'NoiseEstTemplate': (lambda d, P: clean.NoiseEstTemplate(CONTEXT, d, P), clean.NoiseEst, False,
                         'dtype', ((2, 16, 16), 0.25)),
    'MaskThresholdTemplate': (lambda d, P: mask.MaskThresholdTemplate(CONTEXT, d, P, parameters.CLEAN_I),
                              mask.MaskThreshold, False, 'dtype', ((2, 16, 16), 0.25)),
    'PrimaryBeamTemplate': (lambda d, P: primary_beam.PrimaryBeamTemplate(CONTEXT, d, P),
                            primary_beam.PrimaryBeam, False, 'dtype', ((2, 16, 16),)),
    'PredictTemplate': (lambda d, P: predict.PredictTemplate(CONTEXT, d, P), None, False,
                        'real_dtype', None),
    'MultiScaleCleanTemplate': (
        lambda d, P: multiscale.MultiScaleCleanTemplate(CONTEXT, _clean_parameters(), SCALES, d, P),
        multiscale.MultiScaleClean, False, 'dtype', (_image_parameters(2),)),
    'CleanTemplate': (lambda d, P: clean.CleanTemplate(CONTEXT, _clean_parameters(), d, P), None,
                      False, 'dtype', None),
    'FourierBeamTemplate': (lambda d, P: beam.FourierBeamTemplate(CONTEXT, d), beam.FourierBeam,
                            False, 'dtype', ((16, 16),)),
}


@pytest.mark.parametrize('name', sorted(TEMPLATES))
def test_template(name):
    make, operator, float64, dtype_name, args = TEMPLATES[name]
    template = make(np.float32, 2)
    assert type(template).__name__ == name
    assert template.context is CONTEXT
    assert getattr(template, dtype_name) == np.dtype(np.float32)
    assert isinstance(getattr(template, dtype_name), np.dtype)
    if name not in ('LayerToImageTemplate', 'ImageToLayerTemplate', 'FourierBeamTemplate'):
        assert template.num_polarizations == 2
    both = '{}: only float32 and float64 are supported by the HIP path, not {}'
    only = '{}: only float32 is supported by the HIP path, not {}'
    with pytest.raises(ValueError) as info:
        make(np.float16, 2)
    assert str(info.value) == (both if float64 else only).format(name, 'float16')
    if float64:
        assert getattr(make(np.float64, 2), dtype_name) == np.dtype(np.float64)
    else:
        with pytest.raises(ValueError) as info:
            make(np.float64, 2)
        assert str(info.value) == only.format(name, 'float64')
    if operator is not None:
        op = template.instantiate(QUEUE, *args)
        assert type(op) is operator and op.template is template and op.command_queue is QUEUE


def test_templates_with_more_or_less():
    t = clean._UpdateTilesTemplate(CONTEXT, np.float32, 2, parameters.CLEAN_SUMSQ)
    assert (t.mode, t.tilex, t.tiley, t.num_polarizations) == (parameters.CLEAN_SUMSQ, 32, 32, 2)
    assert type(t.instantiate(QUEUE, (2, 64, 64), 0.25)) is clean._UpdateTiles
    with pytest.raises(ValueError, match='^_UpdateTilesTemplate: only float32 is supported'):
        clean._UpdateTilesTemplate(CONTEXT, np.float64, 2, parameters.CLEAN_I)
    assert mask.MaskThresholdTemplate(CONTEXT, np.float32, 1, parameters.CLEAN_SUMSQ).mode == \
        parameters.CLEAN_SUMSQ
    with pytest.raises(ValueError, match='^Invalid mode 7$'):
        mask.MaskThresholdTemplate(CONTEXT, np.float32, 1, 7)
    with pytest.raises(ValueError, match='^1 to 4 polarizations, not 5$'):
        primary_beam.PrimaryBeamTemplate(CONTEXT, np.float32, 5)
    with pytest.raises(ValueError, match='^multi-scale CLEAN runs in mode CLEAN_I only$'):
        multiscale.MultiScaleCleanTemplate(CONTEXT, _clean_parameters(mode=parameters.CLEAN_SUMSQ),
                                           SCALES, np.float32, 1)
    assert predict.PredictTemplate(CONTEXT, np.float32, 4).wgs == 256
    grid_image = image.GridImageTemplate(CONTEXT, np.float64, {'own_transform': False})
    assert (grid_image.real_dtype, grid_image.real_transform, grid_image.own_transform) == \
        (np.dtype(np.float64), True, False)
    assert type(grid_image.layer_to_image) is image.LayerToImageTemplate
    assert type(grid_image.image_to_layer) is image.ImageToLayerTemplate
    with pytest.raises(ValueError, match='^GridImageTemplate: only float32 and float64 are'):
        image.GridImageTemplate(CONTEXT, np.float16)
    for cls, op, args in ((weight.GridWeightsTemplate, weight.GridWeights, ((3, 8, 8), 100)),
                          (weight.DensityWeightsTemplate, weight.DensityWeights, ((3, 8, 8),))):
        template = cls(CONTEXT, 3)
        assert template.context is CONTEXT and template.num_polarizations == 3
        assert type(template.instantiate(QUEUE, *args)) is op
        with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
            template.instantiate(QUEUE, (2,) + args[0][1:], *args[1:])
    assert type(weight.MeanWeightTemplate(CONTEXT).instantiate(QUEUE, (3, 8, 8))) is weight.MeanWeight
    assert type(mask.MaskDilateTemplate(CONTEXT).instantiate(QUEUE, (8, 8))) is mask.MaskDilate


#: operator: (its template for P polarizations, arguments of instantiate after the queue as a
#: function of the image shape and the border, whether it checks the dimensions / the border)
OPERATORS = {
    'Scale': (lambda P: image.ScaleTemplate(CONTEXT, np.float32, P), lambda s, b: (s,), True, False),
    'AddImage': (lambda P: image.AddImageTemplate(CONTEXT, np.float64, P), lambda s, b: (s,), True,
                 False),
    'ApplyPrimaryBeam': (lambda P: image.ApplyPrimaryBeamTemplate(CONTEXT, np.float32, P),
                         lambda s, b: (s, 0.1, 0.0), True, False),
    'PrimaryBeam': (lambda P: primary_beam.PrimaryBeamTemplate(CONTEXT, np.float32, P),
                    lambda s, b: (s,), True, False),
    'PsfPatch': (lambda P: clean.PsfPatchTemplate(CONTEXT, np.float32, P), lambda s, b: (s,), False,
                 False),
    'NoiseEst': (lambda P: clean.NoiseEstTemplate(CONTEXT, np.float32, P), lambda s, b: (s, b), False,
                 True),
    '_UpdateTiles': (lambda P: clean._UpdateTilesTemplate(CONTEXT, np.float32, P, parameters.CLEAN_I),
                     lambda s, b: (s, b), False, True),
    '_FindPeak': (lambda P: clean._FindPeakTemplate(CONTEXT, np.float32, P),
                  lambda s, b: (s, (1, 1)), False, False),
    '_SubtractPsf': (lambda P: clean._SubtractPsfTemplate(CONTEXT, np.float32, P),
                     lambda s, b: (0.1, s, s), False, False),
    'MaskThreshold': (lambda P: mask.MaskThresholdTemplate(CONTEXT, np.float32, P, parameters.CLEAN_I),
                      lambda s, b: (s, b), False, True),
}


@pytest.mark.parametrize('name', sorted(OPERATORS))
def test_operator_shape_errors(name):
    make, args, dimensions, border = OPERATORS[name]
    template = make(2)
    op = template.instantiate(QUEUE, *args((2, 16, 16), 0.25))
    assert type(op).__name__ == name
    with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
        template.instantiate(QUEUE, *args((3, 16, 16), 0.25))
    if dimensions:
        with pytest.raises(ValueError, match='^Wrong number of dimensions in shape$'):
            template.instantiate(QUEUE, *args((2, 16), 0.25))
    if border:
        assert op.border_pixels == 4
        with pytest.raises(ValueError, match='^Border must be less than half the image size$'):
            template.instantiate(QUEUE, *args((2, 16, 16), 0.5))


def test_operator_shape_errors_of_the_rest():
    with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
        clean._SubtractPsfTemplate(CONTEXT, np.float32, 2).instantiate(
            QUEUE, 0.1, (2, 16, 16), (1, 16, 16))
    template = multiscale.MultiScaleCleanTemplate(CONTEXT, _clean_parameters(), SCALES, np.float32, 2)
    assert template.instantiate(QUEUE, _image_parameters(2)).border_pixels == 16
    with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
        template.instantiate(QUEUE, _image_parameters(3))
    with pytest.raises(ValueError, match='^Border must be less than half the image size$'):
        multiscale.MultiScaleCleanTemplate(CONTEXT, _clean_parameters(0.5), SCALES, np.float32,
                                           2).instantiate(QUEUE, _image_parameters(2))
    # (the numpy twin takes any border)
    host = np.zeros((1, 64, 64), np.float32)
    host[0, 32, 32] = 1
    twin = multiscale.MultiScaleCleanHost(SCALES, 0.25, 0.1, parameters.CLEAN_I, host, host.copy(),
                                          host.copy())
    assert twin.border_pixels == 16
    predictor = predict.PredictTemplate(CONTEXT, np.float32, 2)
    with pytest.raises(ValueError, match='^Mismatch in number of polarizations$'):
        predictor.instantiate(QUEUE, _image_parameters(3), None, 10, 10)


# ---- which entry point -----------------------------------------------------------------------
class RecordingLib:
    """Every attribute is a function that records its call and returns 0 (or ``answers[name]``)."""
    def __init__(self, **answers):
        self.calls = []
        self.answers = answers

    def __getattr__(self, name):
        if not name.startswith('kimg_'):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return self.answers.get(name, 0)
        return call


def _patch_lib(monkeypatch, fake):
    for module in (image_plane, image):
        monkeypatch.setattr(module, 'lib', lambda: fake)


def test_masked_call(monkeypatch):
    fake = RecordingLib()
    _patch_lib(monkeypatch, fake)
    image_plane.masked_call('kimg_find_peak', None, QUEUE, 1, 2.5, 'three')
    assert fake.calls == [('kimg_find_peak', (1, 2.5, 'three'))]
    allowed = FakeArray(0x7000, (5, 9), np.uint8)
    image_plane.masked_call('kimg_find_peak', allowed, QUEUE, 1, 2.5, 'three')
    assert fake.calls[1] == ('kimg_find_peak_masked', (1, 2.5, 'three', 0x7000, 9))
    assert allowed.used == [QUEUE]
    failing = RecordingLib(kimg_update_tiles_masked=EINVAL)
    _patch_lib(monkeypatch, failing)
    monkeypatch.setattr(_lib, 'error_string', lambda code: 'bad argument')
    with pytest.raises(_lib.KimgError, match='^kimg_update_tiles_masked failed') as info:
        image_plane.masked_call('kimg_update_tiles', allowed, QUEUE)
    assert info.value.code == EINVAL


def test_masked_prototypes_are_the_unmasked_ones_plus_the_mask():
    for name in ('kimg_update_tiles', 'kimg_find_peak', 'kimg_clean_cycles'):
        restype, args = _lib.PROTOTYPES[name]
        assert _lib.PROTOTYPES[name + '_masked'] == (restype, args + [_lib.P, _lib.L])


PAIRS = ['kimg_grid_to_layer', 'kimg_layer_to_grid', 'kimg_layer_to_image', 'kimg_image_to_layer',
         'kimg_scale', 'kimg_add_image', 'kimg_apply_primary_beam']


@pytest.mark.parametrize('name', PAIRS)
def test_precision_call(name):
    lib = _lib.lib()
    fn, called = image_plane.precision_call(name, np.float32)
    assert called == name and fn is getattr(lib, name)
    fn, called = image_plane.precision_call(name, np.dtype(np.float64))
    assert called == name + '_f64' and fn is getattr(lib, name + '_f64')
    with pytest.raises(ValueError):
        image_plane.precision_call(name, np.float16)


def test_precision_call_unknown_pair():
    for name in ('kimg_grid', 'kimg_fourier_beam', 'kimg_scale_device', 'kimg_scale_f64'):
        with pytest.raises(ValueError, match='has no float64 form'):
            image_plane.precision_call(name, np.float64)


# ---- the route of GridToImage and ImageToGrid ------------------------------------------------
class FakePlan:
    shape = (64, 64)

    def __init__(self):
        self.executed = 0
        self.real_plans = 0

    def execute(self, queue, layer, inverse):
        self.executed += 1

    def real_plan(self):
        self.real_plans += 1
        return types.SimpleNamespace(execute_in_place=lambda *args, **kwargs: None)


#: (w, real_transform, own_transform, the library supports the sizes) -> the float32 route, read off
#: the nested ifs of the two _run methods as they stood; float64 is 'float64' in all 16 rows
FLOAT32_ROUTES = {
    (0, True, True, True): 'own_real',
    (0, True, True, False): 'plan_real',
    (0, True, False, True): 'plan_real',
    (0, True, False, False): 'plan_real',
    (0, False, True, True): 'plain',
    (0, False, True, False): 'plain',
    (0, False, False, True): 'plain',
    (0, False, False, False): 'plain',
    (1.5, True, True, True): 'own_w',
    (1.5, True, True, False): 'plain',
    (1.5, True, False, True): 'plain',
    (1.5, True, False, False): 'plain',
    (1.5, False, True, True): 'plain',
    (1.5, False, True, False): 'plain',
    (1.5, False, False, True): 'plain',
    (1.5, False, False, False): 'plain',
}
#: the first launch of every route, per direction
FIRST_CALL = {
    'grid_to_image': {'float64': 'kimg_grid_to_layer_f64', 'own_real': 'kimg_grid_to_image_real',
                      'plan_real': 'kimg_grid_to_half_layer', 'own_w': 'kimg_grid_to_image_w',
                      'plain': 'kimg_grid_to_layer'},
    'image_to_grid': {'float64': 'kimg_image_to_layer_f64', 'own_real': 'kimg_image_to_grid_real',
                      'plan_real': 'kimg_image_to_real_layer', 'own_w': 'kimg_image_to_grid_w',
                      'plain': 'kimg_image_to_layer'},
}


@pytest.mark.parametrize('direction', sorted(FIRST_CALL))
def test_grid_image_routes(monkeypatch, direction):
    rows = 0
    for dtype, (w, real, own, supported) in itertools.product((np.float32, np.float64),
                                                              FLOAT32_ROUTES):
        expected = 'float64' if dtype == np.float64 else FLOAT32_ROUTES[w, real, own, supported]
        fake = RecordingLib(kimg_grid_image_real_supported=int(supported))
        _patch_lib(monkeypatch, fake)
        template = image.GridImageTemplate(CONTEXT, dtype, {'real_transform': real,
                                                            'own_transform': own})
        plan = FakePlan()
        make = getattr(template, 'instantiate_' + direction)
        op = make(QUEUE, (2, 48, 48), 1e-3, -32e-3, plan)
        cdtype = np.complex64 if dtype == np.float32 else np.complex128
        op.bind(grid=FakeArray(0x10000, (2, 48, 48), cdtype),
                layer=FakeArray(0x20000, (64, 64), cdtype),
                image=FakeArray(0x30000, (2, 64, 64), dtype),
                kernel1d=FakeArray(0x40000, (64,), dtype))
        op.set_w(w)
        op.overwrite_next = True
        if hasattr(op, '_route'):       # (what decides it now; the launches below are the proof)
            assert op._route() == expected
        del fake.calls[:]
        op()
        launches = [name for name, _ in fake.calls if name != 'kimg_grid_image_real_supported']
        assert launches[0] == FIRST_CALL[direction][expected]
        # one launch per polarization on the own routes, two on the others
        assert len(launches) == (2 if expected in ('own_real', 'own_w') else 4)
        assert plan.real_plans == (1 if expected == 'plan_real' else 0)
        assert (op._real_plan is not None) == (expected == 'plan_real')
        assert plan.executed == (2 if expected in ('float64', 'plain') else 0)
        # only grid -> image on its own transforms takes the flag (and writes instead of adding)
        consumed = direction == 'grid_to_image' and expected in ('own_real', 'own_w')
        assert op.overwrite_next is (not consumed)
        if consumed:
            accumulate = fake.calls[-1][1][9 if expected == 'own_real' else 10]
            assert accumulate == 0
            op()
            assert fake.calls[-1][1][9 if expected == 'own_real' else 10] == 1
        if direction == 'grid_to_image':
            assert op.can_overwrite() is (expected in ('own_real', 'own_w'))
        rows += 1
    assert rows == 32


# ---- return codes of csrc/image.hip ------------------------------------------------------------
A, B, C = 0x1000, 0x2000, 0x3000      # non-null "device pointers": no case below reaches a launch


def _cases(good, changes):
    """``good`` with one argument replaced, per entry of ``changes``: (index, value, code)."""
    out = []
    for index, value, code in changes:
        args = list(good)
        args[index] = value
        out.append((tuple(args), code))
    return out


def _grid_layer(layer_at, grid_at, layer_size_at, stride_at, grid_size_at, good):
    return _cases(good, [
        (layer_at, None, EINVAL), (grid_at, None, EINVAL),
        (layer_size_at, 0, EINVAL), (grid_size_at, 0, EINVAL),
        (layer_size_at, 63, EINVAL), (grid_size_at, 47, EINVAL),
        (grid_size_at, 66, EINVAL),                         # grid_size > layer_size
        (stride_at, 47, EINVAL)])


def _layer_image(pointers, stride_at, size_at, good):
    return _cases(good, [(at, None, EINVAL) for at in pointers] + [
        (size_at, 0, EINVAL), (size_at, 63, EINVAL), (stride_at, 63, EINVAL)])


FACTORS32 = (ctypes.c_float * 4)(1, 1, 1, 1)
FACTORS64 = (ctypes.c_double * 4)(1, 1, 1, 1)

#: float32 name -> (arguments, expected code) rows; the *_f64 twin takes the same rows
IMAGE_HIP_ROWS = {
    'kimg_grid_to_layer': _grid_layer(0, 2, 1, 3, 4, (A, 64, B, 48, 48, None)),
    'kimg_layer_to_grid': _grid_layer(3, 0, 4, 1, 2, (A, 48, 48, B, 64, None)),
    'kimg_layer_to_image': _layer_image((0, 2, 4), 1, 3, (A, 64, B, 64, C, 1.0, 0.0, 0.0, None)),
    'kimg_image_to_layer': _layer_image((0, 1, 4), 2, 3, (A, B, 64, 64, C, 1.0, 0.0, 0.0, None)),
    'kimg_scale': _cases((A, 8, 64, 8, 8, 2, 'factors', None), [
        (0, None, EINVAL), (6, None, EINVAL), (3, 0, EINVAL), (4, 0, EINVAL), (1, 7, EINVAL),
        (5, 0, EUNSUPPORTED), (5, 5, EUNSUPPORTED)]),
    # (a polarization count above 4 is accepted by the next two: that would launch)
    'kimg_add_image': _cases((A, 8, 64, B, 8, 64, 8, 8, 2, None), [
        (0, None, EINVAL), (3, None, EINVAL), (6, 0, EINVAL), (7, 0, EINVAL), (1, 7, EINVAL),
        (4, 7, EINVAL), (8, 0, EINVAL)]),
    'kimg_apply_primary_beam': _cases((A, 8, 64, B, 8, 8, 8, 2, 0.1, 0.0, None), [
        (0, None, EINVAL), (3, None, EINVAL), (5, 0, EINVAL), (6, 0, EINVAL), (1, 7, EINVAL),
        (4, 7, EINVAL), (7, 0, EINVAL)]),
}
FLOAT32_ONLY_ROWS = {
    'kimg_scale_device': _cases((A, 8, 64, 8, 8, 2, B, None), [
        (0, None, EINVAL), (6, None, EINVAL), (3, 0, EINVAL), (4, 0, EINVAL), (1, 7, EINVAL),
        (5, 0, EUNSUPPORTED), (5, 5, EUNSUPPORTED)]),
    'kimg_pixel_reciprocal': _cases((A, 8, 64, 8, 8, 2, 4, 4, B, None), [
        (0, None, EINVAL), (8, None, EINVAL), (3, 0, EINVAL), (4, 0, EINVAL), (6, -1, EINVAL),
        (6, 8, EINVAL), (7, -1, EINVAL), (7, 8, EINVAL), (1, 7, EINVAL),
        (5, 0, EUNSUPPORTED), (5, 5, EUNSUPPORTED)]),
}


def _answers(name, rows, factors):
    fn = getattr(_lib.lib(), name)
    return [fn(*[factors if a == 'factors' else a for a in args]) for args, _ in rows]


@pytest.mark.parametrize('name', sorted(IMAGE_HIP_ROWS))
def test_image_hip_return_codes_in_both_precisions(name):
    rows = IMAGE_HIP_ROWS[name]
    expected = [code for _, code in rows]
    single = _answers(name, rows, FACTORS32)
    double = _answers(name + '_f64', rows, FACTORS64)
    assert single == expected
    assert double == single


@pytest.mark.parametrize('name', sorted(FLOAT32_ONLY_ROWS))
def test_image_hip_return_codes_float32_only(name):
    rows = FLOAT32_ONLY_ROWS[name]
    assert _answers(name, rows, None) == [code for _, code in rows]


# ---- on the device: the public classes against the raw entry points -----------------------------
#: (dtype, w, tuning, the route that must have run)
DEVICE_ROWS = [
    (np.float64, 1.5, {}, 'float64'),
    (np.float32, 0, {}, 'own_real'),
    (np.float32, 0, {'own_transform': False}, 'plan_real'),
    (np.float32, 1.5, {}, 'own_w'),
    (np.float32, 1.5, {'own_transform': False, 'real_transform': False}, 'plain'),
]


def _raw_grid_to_image(route, q, plan, grid, layer, image, k1d, scale, bias, w, accumulate):
    """The launches of GridToImage._run, spelled out per route as that method made them."""
    lib = _lib.lib()
    G, Gg = 64, 48
    nbytes = layer.tensor.numel() * layer.tensor.element_size()
    for pol in range(grid.shape[0]):
        g = grid.ptr + pol * Gg * Gg * grid.dtype.itemsize
        i = image.ptr + pol * G * G * image.dtype.itemsize
        if route in ('float64', 'plain'):
            suffix = '_f64' if route == 'float64' else ''
            _lib.check(getattr(lib, 'kimg_grid_to_layer' + suffix)(layer.ptr, G, g, Gg, Gg, q.handle), '')
            plan.execute(q, layer, inverse=True)
            _lib.check(getattr(lib, 'kimg_layer_to_image' + suffix)(
                i, G, layer.ptr, G, k1d.ptr, scale, bias, w, q.handle), '')
        elif route == 'own_real':
            _lib.check(lib.kimg_grid_to_image_real(i, G, G, g, Gg, Gg, k1d.ptr, scale, bias,
                                                   accumulate, layer.ptr, nbytes, q.handle), '')
        elif route == 'own_w':
            _lib.check(lib.kimg_grid_to_image_w(i, G, G, g, Gg, Gg, k1d.ptr, scale, bias, float(w),
                                                accumulate, layer.ptr, nbytes, q.handle), '')
        else:
            _lib.check(lib.kimg_grid_to_half_layer(layer.ptr, G, g, Gg, Gg, q.handle), '')
            plan.real_plan().execute_in_place(q, layer)
            _lib.check(lib.kimg_real_layer_to_image(i, G, layer.ptr, G + 2, G, k1d.ptr, scale, bias,
                                                    q.handle), '')


def _raw_image_to_grid(route, q, plan, grid, layer, image, k1d, scale, bias, w):
    lib = _lib.lib()
    G, Gg = 64, 48
    nbytes = layer.tensor.numel() * layer.tensor.element_size()
    for pol in range(grid.shape[0]):
        g = grid.ptr + pol * Gg * Gg * grid.dtype.itemsize
        i = image.ptr + pol * G * G * image.dtype.itemsize
        if route in ('float64', 'plain'):
            suffix = '_f64' if route == 'float64' else ''
            _lib.check(getattr(lib, 'kimg_image_to_layer' + suffix)(
                layer.ptr, i, G, G, k1d.ptr, scale, bias, w, q.handle), '')
            plan.execute(q, layer, inverse=False)
            _lib.check(getattr(lib, 'kimg_layer_to_grid' + suffix)(g, Gg, Gg, layer.ptr, G, q.handle), '')
        elif route == 'own_real':
            _lib.check(lib.kimg_image_to_grid_real(g, Gg, Gg, i, G, G, k1d.ptr, scale, bias,
                                                   layer.ptr, nbytes, q.handle), '')
        elif route == 'own_w':
            _lib.check(lib.kimg_image_to_grid_w(g, Gg, Gg, i, G, G, k1d.ptr, scale, bias, float(w),
                                                layer.ptr, nbytes, q.handle), '')
        else:
            _lib.check(lib.kimg_image_to_real_layer(layer.ptr, G + 2, i, G, G, k1d.ptr, scale, bias,
                                                    q.handle), '')
            plan.real_plan().execute_in_place(q, layer, inverse=False)
            _lib.check(lib.kimg_half_layer_to_grid(g, Gg, Gg, layer.ptr, G, q.handle), '')


@pytest.mark.gpu
def test_grid_image_round_trip_is_the_raw_calls_to_the_byte():
    ctx = accel.create_some_context()
    q = ctx.create_command_queue()
    rng = np.random.RandomState(7)
    P, G, Gg = 2, 64, 48
    scale, bias = 1e-3, -0.5 * G * 1e-3
    for dtype, w, tuning, route in DEVICE_ROWS:
        overwrite = route == 'own_real'     # this row once more with overwrite_next set
        cdtype = np.complex64 if dtype == np.float32 else np.complex128
        grid_host = (rng.standard_normal((P, Gg, Gg)) + 1j * rng.standard_normal((P, Gg, Gg))).astype(cdtype)
        k1d_host = (1.0 + 0.5 * rng.rand(G)).astype(dtype)
        start_host = rng.standard_normal((P, G, G)).astype(dtype)
        template = image.GridImageTemplate(ctx, dtype, tuning)
        plan = template.make_fft_plan((G, G))
        for flag in ((False, True) if overwrite else (False,)):
            results = []
            for public in (True, False):
                arrays = {name: accel.DeviceArray(ctx, shape, dt, queue=q) for name, shape, dt in (
                    ('grid', (P, Gg, Gg), cdtype), ('layer', (G, G), cdtype),
                    ('image', (P, G, G), dtype), ('kernel1d', (G,), dtype),
                    ('grid_out', (P, Gg, Gg), cdtype))}
                arrays['grid'].set(q, grid_host)
                arrays['kernel1d'].set(q, k1d_host)
                arrays['image'].set(q, start_host)
                arrays['layer'].zero(q)
                arrays['grid_out'].zero(q)
                if public:
                    g2i = template.instantiate_grid_to_image(q, (P, Gg, Gg), scale, bias, plan)
                    i2g = template.instantiate_image_to_grid(q, (P, Gg, Gg), scale, bias, plan)
                    g2i.bind(grid=arrays['grid'], layer=arrays['layer'], image=arrays['image'],
                             kernel1d=arrays['kernel1d'])
                    i2g.bind(grid=arrays['grid_out'], layer=arrays['layer'], image=arrays['image'],
                             kernel1d=arrays['kernel1d'])
                    g2i.set_w(w)
                    i2g.set_w(w)
                    g2i.overwrite_next = flag
                    if hasattr(g2i, '_route'):
                        assert g2i._route() == route and i2g._route() == route
                    assert g2i.can_overwrite() is (route in ('own_real', 'own_w'))
                    g2i()
                    assert g2i.overwrite_next is False or route not in ('own_real', 'own_w')
                    i2g()
                else:
                    _raw_grid_to_image(route, q, plan, arrays['grid'], arrays['layer'],
                                       arrays['image'], arrays['kernel1d'], scale, bias, w,
                                       0 if flag else 1)
                    _raw_image_to_grid(route, q, plan, arrays['grid_out'], arrays['layer'],
                                       arrays['image'], arrays['kernel1d'], scale, bias, w)
                results.append((arrays['image'].get(q).copy(), arrays['grid_out'].get(q).copy()))
            (image_a, grid_a), (image_b, grid_b) = results
            assert image_a.tobytes() == image_b.tobytes(), (route, flag)
            assert grid_a.tobytes() == grid_b.tobytes(), (route, flag)
            assert np.isfinite(image_a).all() and np.abs(grid_a).max() > 0
            if flag:        # written, not added to the non-zero start
                assert not np.array_equal(image_a, start_host)
