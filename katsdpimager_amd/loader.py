"""A minimal visibility loader: arrays in memory or in a ``.npz`` file, delivered
the way the reference's loaders deliver them.

The reference reads measurement sets (python-casacore) and katdal files; both are outside the hot
path and their libraries are not available here.  What the path needs from a loader is the *shape
of the stream*: ``data_iter`` yields blocks of at most ``max_chunk_vis`` visibilities (over the
selected channels), each block **sorted by baseline** with a stable sort so that the
preprocessor's adjacent-merge compression finds runs (loader_ms.py:377-467; interface
loader_core.py:149-200), as dicts with ``uvw`` [N][3] metres, ``weights`` / ``vis``
[channel][N][polarization], optional ``feed_angle1/2`` [N], ``progress`` and ``total``.
:func:`preprocess_visibilities` is the loop of frontend.preprocess_visibilities
(frontend.py:40-84) around ``VisibilityCollectorDevice.add``.

File layout of :class:`LoaderArrays.save` / ``load``: ``uvw`` f4 [R][3] (metres), ``vis`` c8
[R][C][P], ``weights`` f4 [R][C][P], ``baseline`` i4 [R] (any integer that identifies the antenna
pair), ``frequency`` f8 [C] (Hz), ``polarizations`` i4 [P] (the reference's polarization
enumeration), ``phase_centre`` f8 [2] (RA, Dec in radians), ``antenna_diameter`` f8,
``longest_baseline`` f8 (metres), and optionally ``feed_angle1`` / ``feed_angle2`` f4 [R].  Rows
are in time order, as a correlator writes them.
"""
import numpy as np

from . import parameters

_LIGHTSPEED = 299792458.0


class LoaderArrays:
    """Loader over arrays held in memory (see the module docstring for their meaning)."""

    def __init__(self, uvw, vis, weights, baseline, frequency, polarizations, phase_centre=(0.0, 0.0),
                 antenna_diameter=13.5, longest_baseline=None, feed_angle1=None, feed_angle2=None):
        self.uvw = np.ascontiguousarray(uvw, np.float32)
        self.vis = np.asarray(vis, np.complex64)
        self.weights = np.asarray(weights, np.float32)
        self.baseline = np.asarray(baseline)
        self.frequencies = np.atleast_1d(np.asarray(frequency, np.float64))
        self._polarizations = [int(p) for p in polarizations]
        self._phase_centre = (float(phase_centre[0]), float(phase_centre[1]))
        self._antenna_diameter = float(antenna_diameter)
        rows = len(self.uvw)
        if self.uvw.shape != (rows, 3) or self.vis.shape != self.weights.shape \
                or self.vis.shape != (rows, len(self.frequencies), len(self._polarizations)) \
                or self.baseline.shape != (rows,):
            raise ValueError('inconsistent array shapes')
        if longest_baseline is None:
            longest_baseline = float(np.sqrt((self.uvw.astype(np.float64) ** 2).sum(axis=1)).max()) \
                if rows else 0.0
        self._longest_baseline = float(longest_baseline)
        self.feed_angle1 = None if feed_angle1 is None else np.asarray(feed_angle1, np.float32)
        self.feed_angle2 = None if feed_angle2 is None else np.asarray(feed_angle2, np.float32)
        if (self.feed_angle1 is None) != (self.feed_angle2 is None):
            raise ValueError('feed angles come in pairs')

    # ---- persistence -------------------------------------------------------------------------
    _FIELDS = ('uvw', 'vis', 'weights', 'baseline')

    def save(self, filename):
        extra = {}
        if self.feed_angle1 is not None:
            extra = dict(feed_angle1=self.feed_angle1, feed_angle2=self.feed_angle2)
        np.savez(filename, uvw=self.uvw, vis=self.vis, weights=self.weights, baseline=self.baseline,
                 frequency=self.frequencies, polarizations=np.array(self._polarizations, np.int32),
                 phase_centre=np.array(self._phase_centre), antenna_diameter=self._antenna_diameter,
                 longest_baseline=self._longest_baseline, **extra)

    @classmethod
    def load(cls, filename):
        with np.load(filename) as f:
            return cls(f['uvw'], f['vis'], f['weights'], f['baseline'], f['frequency'],
                       f['polarizations'], f['phase_centre'], float(f['antenna_diameter']),
                       float(f['longest_baseline']),
                       f['feed_angle1'] if 'feed_angle1' in f.files else None,
                       f['feed_angle2'] if 'feed_angle2' in f.files else None)

    @classmethod
    def match(cls, filename):
        """loader_core.py:32"""
        return filename.lower().endswith('.npz')

    # ---- the LoaderBase interface the path uses (loader_core.py:36-239) ------------------------
    def antenna_diameter(self):
        return self._antenna_diameter

    def longest_baseline(self):
        return self._longest_baseline

    def array_parameters(self):
        return parameters.ArrayParameters(self._antenna_diameter, self._longest_baseline)

    def num_channels(self):
        return len(self.frequencies)

    def frequency(self, channel):
        return float(self.frequencies[channel])

    def wavelength(self, channel):
        return _LIGHTSPEED / self.frequency(channel)

    def phase_centre(self):
        return self._phase_centre

    def polarizations(self):
        return list(self._polarizations)

    def has_feed_angles(self):
        return self.feed_angle1 is not None

    def channel_enabled(self, channel):
        return True

    def data_iter(self, start_channel, stop_channel, max_chunk_vis=None):
        """loader_core.py:149-200 with the block shaping of loader_ms.py:377-467: at most
        ``max_chunk_vis`` visibilities (rows x channels) per block, rows of a block in a stable
        sort by baseline, channel axis first."""
        if not 0 <= start_channel < stop_channel <= self.num_channels():
            raise ValueError('bad channel range')
        rows = len(self.uvw)
        num_channels = stop_channel - start_channel
        if max_chunk_vis is None:
            max_chunk_vis = max(rows * num_channels, 1)
        max_chunk_rows = max(1, max_chunk_vis // num_channels)
        for start in range(0, rows, max_chunk_rows):
            end = min(rows, start + max_chunk_rows)
            order = np.argsort(self.baseline[start:end], kind='stable') + start
            ret = dict(
                uvw=self.uvw[order],
                weights=np.ascontiguousarray(
                    np.swapaxes(self.weights[order][:, start_channel:stop_channel], 0, 1)),
                vis=np.ascontiguousarray(
                    np.swapaxes(self.vis[order][:, start_channel:stop_channel], 0, 1)),
                baselines=self.baseline[order], progress=end, total=rows)
            if self.feed_angle1 is not None:
                ret['feed_angle1'] = self.feed_angle1[order]
                ret['feed_angle2'] = self.feed_angle2[order]
            yield ret

    def close(self):
        pass


def load(filename):
    """loader.load (loader.py:13-33) for the one format this package reads."""
    if not LoaderArrays.match(filename):
        raise ValueError('{}: only .npz visibility files are supported'.format(filename))
    return LoaderArrays.load(filename)


def data_iter(dataset, vis_limit, vis_load, start_channel, stop_channel):
    """loader.data_iter (loader.py:36-59): stop after ``vis_limit`` rows."""
    remaining = vis_limit
    for chunk in dataset.data_iter(start_channel, stop_channel, vis_load):
        if remaining is not None and remaining < len(chunk['uvw']):
            for key in ('uvw', 'baselines', 'feed_angle1', 'feed_angle2'):
                if key in chunk:
                    chunk[key] = chunk[key][:remaining]
            for key in ('weights', 'vis'):
                chunk[key] = chunk[key][:, :remaining]
            chunk['progress'] = chunk['total']
        yield chunk
        if remaining is not None:
            remaining -= len(chunk['uvw'])
            if remaining <= 0:
                return


def preprocess_visibilities(dataset, collector, start_channel, stop_channel, polarization_matrices,
                            vis_load=32 * 1048576, vis_limit=None, continuum=None,
                            phase_centre=None, continuum_centre=None, spectral=None, statwt=None,
                            rfiflag=None):
    """frontend.preprocess_visibilities (frontend.py:40-84): feed every block of the loader, in
    loader order, to ``collector.add`` (a :class:`~.preprocess.VisibilityCollectorDevice`; its
    conversion and compression kernels run asynchronously on its queue, which plays the role of
    the reference's preprocessing thread).  ``polarization_matrices`` = (mueller_stokes,
    mueller_circular) as ``polarization.polarization_matrices`` returns them.  Closes the
    collector and returns it.

    ``continuum`` (:class:`~.continuum.UVContSubParameters`; new here) takes the continuum out of
    every block before the collector sees it: the block's visibilities and weights are moved to the
    device once, a polynomial is fitted across the line-free channels of every sample and subtracted
    (``continuum.UVContSub`` on the collector's queue), and the collector is handed the device
    arrays.  The mask (and the frequencies, if given) span the loaded channels
    ``start_channel:stop_channel`` -- with ``spectral``, the OUTPUT channels of the filter.  The
    collector then has ``continuum_counts``: the samples (fitted, flagged for want of line-free
    channels) over all blocks.  None (the default) changes nothing.

    ``phase_centre`` = (ra, dec) in radians (new here) images around another direction T than the
    dataset's ``phase_centre()`` O: every block goes to the device once, its visibilities are
    re-phased and its uvw rotated from O to T (``phaseshift.PhaseShift`` on the collector's queue),
    then ``continuum``, if given, runs, and the collector receives the device visibilities, weights
    and new uvw.  ``continuum_centre`` = (ra, dec) (needs ``continuum``) puts the continuum fit, which
    is exact only for a source at the phase centre, on a bright source S elsewhere: visibilities
    only O -> S, the fit, then S -> T on the block's original uvw (T defaults to O, and then no
    coordinates are written); coordinates are never rotated twice.  Either way the collector gets
    ``phase_centre`` = T, for whoever writes the image header.  Feed angles pass unchanged, which is
    valid for shifts small against a radian.

    ``spectral`` (:class:`~.spectral.SpectralParameters`; new here) smooths and averages the channel
    axis of every block on the device (``spectral.SpectralFilter`` on the collector's queue): per
    block the order is the phase shift, if any; the spectral filter; the continuum fit, if any.  The
    loaded channels ``start_channel:stop_channel`` are the filter's input; the collector must have
    been made for its ``spectral.output_channels(stop_channel - start_channel)`` output channels,
    with image and grid parameters of ``spectral.output_frequencies`` (ValueError otherwise, before
    any block is read), and gets ``spectral_counts``: the output samples (kept, flagged for want of
    coverage) over all blocks.  With ``bin`` above 1 there is no ``continuum_centre``: its second
    shift would need the averaged frequencies.

    ``statwt`` (:class:`~.statwt.StatWtParameters`; new here) rescales the weights of every block to
    inverse variances measured from the scatter of its visibilities (``statwt.StatWt`` on the
    collector's queue, fed the block's ``baselines``): per block it runs right after the continuum
    fit and BEFORE the second shift of ``continuum_centre`` -- a shift puts a per-channel phase ramp
    on any continuum left over, and a ramp reads as scatter; what the fit leaves is noise, which does
    not mind the order.  Its mask spans the channels the operator sees, the spectral filter's outputs
    if there is one (ValueError, before any block is read, if it does not fit them).  Groups never
    span blocks.  The collector gets ``statwt_counts``: the (group, polarization) pairs (kept,
    flagged) over all blocks.

    ``rfiflag`` (:class:`~.rfiflag.RFIFlagParameters`; new here) flags interference per sample
    (``rfiflag.RFIFlag`` on the collector's queue, fed the block's ``baselines``): SumThreshold over
    every baseline's time-frequency plane of the block, the weights of the flagged samples set to 0.
    Per block it runs right after the continuum fit, on its residuals, and before ``statwt``, which
    then measures the scatter of what is left.  Its mask spans the channels the operator sees, as
    for ``statwt`` (ValueError, before any block is read, if it does not fit them); groups never
    span blocks.  The collector gets ``rfiflag_counts``: usable samples (kept, flagged) and (group,
    polarization) pairs skipped, over all blocks.  The continuum is not fitted again on the flagged
    residuals.

    With none of the keywords the function is what it was."""
    if continuum_centre is not None and continuum is None:
        raise ValueError('continuum_centre needs continuum')
    if spectral is not None:
        if spectral.bin > 1 and continuum_centre is not None:
            raise ValueError('spectral averaging (bin > 1) cannot be combined with continuum_centre')
        channels_out = spectral.output_channels(stop_channel - start_channel)
        if collector.num_channels != channels_out:
            raise ValueError('the spectral filter gives {} channels, the collector was made for {}'.format(
                channels_out, collector.num_channels))
    if statwt is not None:
        statwt.mask(stop_channel - start_channel if spectral is None else channels_out)
    if rfiflag is not None:
        rfiflag.mask(stop_channel - start_channel if spectral is None else channels_out)
    if continuum is None and phase_centre is None and spectral is None and statwt is None \
            and rfiflag is None:
        try:
            for chunk in data_iter(dataset, vis_limit, vis_load, start_channel, stop_channel):
                collector.add(chunk['uvw'], chunk['weights'], chunk['vis'],
                              chunk.get('feed_angle1'), chunk.get('feed_angle2'), *polarization_matrices)
        finally:
            collector.close()
        return collector
    return _preprocess_device(dataset, collector, start_channel, stop_channel, polarization_matrices,
                              vis_load, vis_limit, continuum, phase_centre, continuum_centre, spectral,
                              statwt, rfiflag)


def _preprocess_device(dataset, collector, start_channel, stop_channel, polarization_matrices,
                       vis_load, vis_limit, continuum, phase_centre, continuum_centre, spectral,
                       statwt=None, rfiflag=None):
    """:func:`preprocess_visibilities` with any of its operators: every block goes to the device
    once and through them on the collector's queue."""
    from . import accel, phaseshift
    from .continuum import UVContSubTemplate
    from .spectral import SpectralFilterTemplate
    from .statwt import StatWtTemplate
    from .rfiflag import RFIFlagTemplate
    queue = collector.queue
    context = queue.context
    shifted = phase_centre is not None or continuum_centre is not None
    channels = stop_channel - start_channel
    try:
        before = after = None
        if shifted:
            origin = tuple(float(x) for x in dataset.phase_centre())
            target = origin if phase_centre is None else tuple(float(x) for x in phase_centre)
            inv_wavelength = phaseshift.inverse_wavelengths(
                [dataset.frequency(channel) for channel in range(start_channel, stop_channel)])

            def shifter(*centres, **kwargs):
                params = phaseshift.PhaseShiftParameters(*centres, **kwargs)
                return phaseshift.PhaseShiftTemplate(context, params).instantiate(queue, inv_wavelength)
            if continuum_centre is not None:
                source = tuple(float(x) for x in continuum_centre)
                before = shifter(origin, source)
                after = shifter(origin, target, from_centre=source)
            else:
                before = shifter(origin, target)
        smooth = None
        if spectral is not None:
            smooth = SpectralFilterTemplate(context, spectral).instantiate(queue, channels)
            channels = smooth.num_channels_out
        subtract = None
        if continuum is not None:
            subtract = UVContSubTemplate(context, continuum).instantiate(queue, channels)
        flag = None
        if rfiflag is not None:
            flag = RFIFlagTemplate(context, rfiflag).instantiate(queue, channels)
        reweight = None
        if statwt is not None:
            reweight = StatWtTemplate(context, statwt).instantiate(queue, channels)
        for chunk in data_iter(dataset, vis_limit, vis_load, start_channel, stop_channel):
            vis = accel.DeviceArray(context, chunk['vis'].shape, np.complex64, queue=queue)
            weights = accel.DeviceArray(context, chunk['weights'].shape, np.float32, queue=queue)
            vis.set(queue, chunk['vis'])
            weights.set(queue, chunk['weights'])
            uvw = chunk['uvw']
            if shifted:
                uvw = accel.DeviceArray(context, chunk['uvw'].shape, np.float32, queue=queue)
                uvw.set(queue, chunk['uvw'])
                if after is None:
                    uvw = before(vis, uvw)
                else:
                    before(vis, uvw, write_uvw=False)
            if smooth is not None:
                vis, weights = smooth(vis, weights)
            if subtract is not None:
                subtract(vis, weights)
            if flag is not None:
                flag(vis, weights, chunk['baselines'])
            if reweight is not None:
                reweight(vis, weights, chunk['baselines'])
            if after is not None:
                if after.template.params.writes_uvw:
                    uvw = after(vis, uvw)
                else:
                    after(vis, uvw, write_uvw=False)
            collector.add(uvw, weights, vis,
                          chunk.get('feed_angle1'), chunk.get('feed_angle2'), *polarization_matrices)
        if smooth is not None:
            collector.spectral_counts = smooth.counts()
        if subtract is not None:
            collector.continuum_counts = subtract.counts()
        if flag is not None:
            collector.rfiflag_counts = flag.counts()
        if reweight is not None:
            collector.statwt_counts = reweight.counts()
        if shifted:
            collector.phase_centre = target
    finally:
        collector.close()
    return collector
