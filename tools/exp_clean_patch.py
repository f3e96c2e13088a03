"""CLEAN minor cycles per second of the device-resident loop for one PSF-patch size and every form of
the loop that takes it (two launches per cycle, one launch, what AUTO chooses), on the
bench's CLEAN image (4096^2, 200 point sources (x) PSF + noise).

    python tools/exp_clean_patch.py [patch height] [patch width] [cycles]"""
import os
import sys
import time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from katsdpimager_amd import _lib as _kl
if os.environ.get('KIMG_VARIANT_LIB'):
    _kl.LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'build_variants',
                                'libkimg_%s.so' % os.environ['KIMG_VARIANT_LIB'])
from katsdpimager_amd import accel, clean, parameters

ph = int(sys.argv[1]) if len(sys.argv) > 1 else 711
pw = int(sys.argv[2]) if len(sys.argv) > 2 else 675
cycles = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
G, P = 4096, 1
ctx = accel.create_some_context()
q = ctx.create_command_queue()
rs = np.random.RandomState(4)
g1 = np.exp(-0.5 * ((np.arange(G) - G // 2) / 6.0) ** 2).astype(np.float32)
psf = np.outer(g1, g1)[None].astype(np.float32)
psf += (0.002 * rs.standard_normal(psf.shape)).astype(np.float32)
psf[:, G // 2, G // 2] = 1.0
sky = (0.01 * rs.standard_normal((P, G, G))).astype(np.float32)
for _ in range(200):
    y, x = rs.randint(100, G - 100, 2)
    sky[:, y - 30:y + 31, x - 30:x + 31] += rs.uniform(0.5, 2.0) * psf[:, G // 2 - 30:G // 2 + 31,
                                                                     G // 2 - 30:G // 2 + 31]


class _IP:      # what CleanTemplate.instantiate reads of the image parameters
    pixels = G

    class fixed:
        polarizations = [0]
        real_dtype = np.float32


cp = parameters.CleanParameters(cycles, 0.1, 0.85, 5.0, 0, 0.01, 0.5, 0.02)
patch = (P, ph, pw)
first = None
for form in ('two_launch', 'one_launch', 'auto'):
    try:
        cl = clean.CleanTemplate(ctx, cp, np.float32, P, {'form': form}).instantiate(q, _IP)
        cl.ensure_all_bound()
        cl.buffer('psf').set(q, psf)
        rates = []
        for rep in range(3):
            cl.buffer('dirty').set(q, sky)
            cl.buffer('model').zero(q)
            cl.reset()
            q.finish()
            t0 = time.perf_counter()
            got = cl.run_cycles(patch, 0.0, cycles)
            q.finish()
            rates.append(len(got) / (time.perf_counter() - t0))
        sig = [(round(float(v), 6), tuple(p)) for v, p, m in got[:50]]
        first = first or sig
        print('%-12s patch %d x %d: %8.0f cycles/s = %.2f us per cycle  (%s)' % (
            form, ph, pw, max(rates), 1e6 / max(rates), 'same components' if sig == first else 'DIFFERENT'))
        del cl
    except Exception as exc:        # noqa: B902
        print('%-12s %s' % (form, exc))
