"""CPU-only tests of what the per-channel operators share (katsdpimager_amd/channel_block.py): the
channel selection against what the three parameter classes returned before they shared it (the
expected values are literals, taken from those classes), the groups of rows, the channel pitch, and
the names that still import from the operators' own modules."""
import types

import numpy as np
import pytest
import torch

from katsdpimager_amd import channel_block, continuum, rfiflag, statwt
from katsdpimager_amd.channel_block import ChannelSelection, channel_pitch, group_offsets

FIT_MASK = [1, 0, 2, 1, 0, 1, 1, 1]

#: how each parameter class is made with a selection; the fit is of order 1
MAKERS = {
    'fit': lambda **kw: continuum.UVContSubParameters(1, **kw),
    'statwt': lambda **kw: statwt.StatWtParameters(2, **kw),
    'rfiflag': lambda **kw: rfiflag.RFIFlagParameters(**kw),
}
SELECTIONS = {
    'fit': lambda **kw: ChannelSelection(order=1, **kw),
    'statwt': lambda **kw: ChannelSelection(**kw),
    'rfiflag': lambda **kw: ChannelSelection(**kw),
}


def _both(which):
    """The parameter class and the bare selection: they must answer alike."""
    return MAKERS[which], SELECTIONS[which]


@pytest.mark.parametrize('which', sorted(MAKERS))
def test_selection_masks(which):
    for make in _both(which):
        mask = make(fit_mask=FIT_MASK).mask(8)
        assert mask.dtype == np.uint8 and mask.tolist() == [1, 0, 1, 1, 0, 1, 1, 1]
        assert make(line_ranges=[(2, 4), (6, 7)]).mask(8).tolist() == [1, 1, 0, 0, 1, 1, 0, 1]
        with pytest.raises(ValueError, match=r'line range \(2, 9\) beyond the 8 channels'):
            make(line_ranges=[(2, 9)]).mask(8)
        with pytest.raises(ValueError, match='fit_mask has 8 entries for 7 channels'):
            make(fit_mask=FIT_MASK).mask(7)
        with pytest.raises(ValueError, match='no channels'):
            make(line_ranges=[]).mask(0)
        with pytest.raises(ValueError, match='bad line range'):
            make(line_ranges=[(3, 2)])
        # the mask handed out is a copy
        selection = make(fit_mask=FIT_MASK)
        selection.mask(8)[:] = 0
        assert selection.mask(8).tolist() == [1, 0, 1, 1, 0, 1, 1, 1]
        assert selection.fit_mask.tolist() == [1, 0, 1, 1, 0, 1, 1, 1] and selection.line_ranges is None
        assert make(line_ranges=[(2, 4)]).line_ranges == [(2, 4)]


def test_selection_neither_spelling():
    for which in ('statwt', 'rfiflag'):
        for make in _both(which):
            assert make().mask(5).tolist() == [1, 1, 1, 1, 1]
            assert make().fit_mask is None and make().line_ranges is None
            with pytest.raises(ValueError, match='at most one of fit_mask and line_ranges may be given'):
                make(fit_mask=FIT_MASK, line_ranges=[(1, 2)])
    for make in _both('fit'):
        with pytest.raises(ValueError, match='exactly one of fit_mask and line_ranges must be given'):
            make()
        with pytest.raises(ValueError, match='exactly one of fit_mask and line_ranges must be given'):
            make(fit_mask=FIT_MASK, line_ranges=[(1, 2)])


def test_selection_too_few_channels():
    for make in (lambda **kw: continuum.UVContSubParameters(3, **kw),
                 lambda **kw: ChannelSelection(order=3, **kw)):
        assert make(line_ranges=[(1, 5)]).mask(8).tolist() == [1, 0, 0, 0, 0, 1, 1, 1]
        with pytest.raises(ValueError, match='order 3 needs 4 line-free channels, 3 remain'):
            make(line_ranges=[(1, 6)]).mask(8)
    with pytest.raises(ValueError, match='order 3 needs 4 line-free channels, 3 remain'):
        continuum.UVContSubParameters(3, fit_mask=[1, 1, 0, 1, 0])
    for make in _both('fit'):
        with pytest.raises(ValueError, match='order 1 needs 2 line-free channels, 0 remain'):
            make(line_ranges=[(0, 8)]).mask(8)
    for which in ('statwt', 'rfiflag'):
        for make in _both(which):
            with pytest.raises(ValueError, match='no line-free channel remains'):
                make(line_ranges=[(0, 8)]).mask(8)
        with pytest.raises(ValueError, match='no line-free channel remains'):
            MAKERS[which](fit_mask=[0, 0, 0])


def test_reprs_keep_their_spelling():
    assert repr(MAKERS['fit'](fit_mask=FIT_MASK)) == \
        'UVContSubParameters(1, fit_mask=[1, 0, 1, 1, 0, 1, 1, 1])'
    assert repr(MAKERS['fit'](line_ranges=[(2, 4)])) == 'UVContSubParameters(1, line_ranges=[(2, 4)])'
    assert repr(MAKERS['statwt'](fit_mask=FIT_MASK)) == \
        'StatWtParameters(2, fit_mask=[1, 0, 1, 1, 0, 1, 1, 1], min_samples=8, chi2_range=(0.0, inf))'
    assert repr(MAKERS['statwt']()) == 'StatWtParameters(2, min_samples=8, chi2_range=(0.0, inf))'
    assert repr(MAKERS['rfiflag'](line_ranges=[(2, 4)])) == (
        "RFIFlagParameters(64, threshold=6.0, rho=1.5, max_window=16, directions='both', "
        "level_iterations=2, level_clip=4.0, extend_freq=0.5, extend_time=0.5, extend_pols=True, "
        "line_ranges=[(2, 4)])")
    assert not hasattr(MAKERS['rfiflag'](), '_spelled')


def test_group_offsets():
    def offsets(baselines, time_bin):
        out = group_offsets(np.asarray(baselines, np.int32), time_bin)
        assert out.dtype == np.int32
        return out.tolist()
    assert offsets([], 4) == [0]                                        # an empty block
    assert offsets([5, 5, 5], 4) == [0, 3]                              # one run shorter than time_bin
    assert offsets([7] * 9, 4) == [0, 4, 8, 9]                          # 2 * time_bin + 1 rows
    # baseline 1 returns later in the block: a new run
    returning = [1, 1, 1, 2, 2, 1, 1, 1, 1, 1]
    assert offsets(returning, 2) == [0, 2, 3, 5, 7, 9, 10]
    assert channel_block._row_groups(group_offsets(np.array(returning), 2)).tolist() == \
        [0, 0, 1, 2, 2, 3, 3, 4, 4, 5]
    with pytest.raises(ValueError):
        group_offsets(np.zeros((2, 2), np.int32), 2)
    with pytest.raises(ValueError):
        group_offsets(np.zeros(3, np.int32), channel_block.MAX_BIN + 1)


def _array(tensor):
    """What channel_pitch reads of a device array."""
    return types.SimpleNamespace(tensor=tensor, shape=tuple(tensor.shape))


def test_channel_pitch():
    dense = torch.zeros((5, 7, 2))
    assert channel_pitch(_array(dense), 'vis') == 14
    padded = torch.zeros((5, 20)).as_strided((5, 7, 2), (20, 2, 1))
    assert channel_pitch(_array(padded), 'vis') == 20
    # a single channel: whatever its stride says, the plane
    assert channel_pitch(_array(torch.zeros((1, 7, 2)).as_strided((1, 7, 2), (3, 2, 1))), 'vis') == 14
    # an empty plane
    assert channel_pitch(_array(torch.zeros((5, 0, 2))), 'vis') == 0
    assert channel_pitch(_array(torch.zeros((5, 7, 0))), 'vis') == 0
    with pytest.raises(ValueError, match=r'weights: the \[row\]\[polarization\] plane must be dense'):
        channel_pitch(_array(torch.zeros((5, 2, 7)).transpose(1, 2)), 'weights')
    with pytest.raises(ValueError, match='vis: channels overlap'):
        channel_pitch(_array(torch.zeros(100).as_strided((5, 7, 2), (13, 2, 1))), 'vis')


def test_integer():
    assert channel_block.integer(np.int64(3), 'n', 1, 4) == 3 and channel_block.integer(4.0, 'n', 1, 4) == 4
    for bad in (0, 5, 2.5, 'x', None, float('inf')):
        with pytest.raises(ValueError, match='n must be an integer'):
            channel_block.integer(bad, 'n', 1, 4)


def test_old_names_still_import():
    from katsdpimager_amd import phaseshift, spectral
    assert statwt.group_offsets is channel_block.group_offsets
    assert statwt._row_groups is channel_block._row_groups
    assert statwt._sum_over_groups is channel_block._sum_over_groups
    assert continuum.MAX_CHANNELS == channel_block.MAX_CHANNELS == 16384
    assert statwt.MAX_BIN == rfiflag.MAX_BIN == channel_block.MAX_BIN == 64
    for module, template, operator, params in (
            (continuum, 'UVContSubTemplate', 'UVContSub', 'UVContSubParameters'),
            (statwt, 'StatWtTemplate', 'StatWt', 'StatWtParameters'),
            (rfiflag, 'RFIFlagTemplate', 'RFIFlag', 'RFIFlagParameters'),
            (spectral, 'SpectralFilterTemplate', 'SpectralFilter', 'SpectralParameters'),
            (phaseshift, 'PhaseShiftTemplate', 'PhaseShift', 'PhaseShiftParameters')):
        cls = getattr(module, template)
        assert issubclass(cls, channel_block.OperatorTemplate)
        assert cls.operator is getattr(module, operator) and cls.params_type is getattr(module, params)
        assert issubclass(cls.operator, channel_block.ChannelOperator)
        with pytest.raises(TypeError, match='params must be ' + params):
            cls(None, object())
    # the shared module imports none of the five
    source = open(channel_block.__file__).read()
    for name in ('continuum', 'statwt', 'rfiflag', 'spectral', 'phaseshift'):
        assert 'import ' + name not in source and 'from .' + name not in source
