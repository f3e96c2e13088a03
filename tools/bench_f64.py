"""Float64 path against float32 on the C2 stream (synth.py: 4096^2, 32 W planes, K = 28, P = 1),
in one process: gridder (stream as generated and a shuffled copy), degridder, grid -> image and
image -> grid at w = 0 and w != 0.  Prints one line per measurement.
python tools/bench_f64.py [--vis N] [--reps R]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _timed(fn, q, reps):
    fn()
    q.finish()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    q.finish()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vis', type=int, default=1 << 22)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    import synth
    from katsdpimager_amd import accel, grid, image, parameters
    ctx = accel.create_some_context()
    q = ctx.create_command_queue()
    obs = synth.make_observation(4096, args.vis, 32, 1, device=ctx.device, cover=0.30)
    n = obs.n_vis
    shuffled = synth.order_shuffled(obs)['obs']
    ip32, gp, ap_ = synth.make_parameters(obs, 1, 28)
    fixed64 = parameters.FixedImageParameters([0], np.float64)
    ip64 = parameters.ImageParameters(fixed64, 1.0, None, obs.wavelength, None,
                                      pixel_size=obs.pixel_size, pixels=obs.pixels)
    print('C2 stream: %d visibilities, 4096^2, 32 W planes, K = 28, P = 1' % n)

    def bind_vis(op, o):
        op.bind(uv=accel.DeviceArray(ctx, (n, 4), np.int16, tensor=o.uv[:n]),
                w_plane=accel.DeviceArray(ctx, (n,), np.int16, tensor=o.w_plane[:n]),
                vis=accel.DeviceArray(ctx, (n, 1), np.complex64, tensor=o.vis[:n].reshape(n, 1)))
        op.num_vis = n

    grids = {}
    for name, ip, tuning, o in (('f64 gridder auto, stream as generated', ip64, {}, obs),
                                ('f64 gridder auto, shuffled', ip64, {}, shuffled),
                                ('f32 gridder mfma, stream as generated', ip32, {'variant': 'mfma'}, obs),
                                ('f32 gridder binned, shuffled', ip32, {'variant': 'binned'}, shuffled)):
        fn = grid.GridderTemplate(ctx, ip.fixed, gp.fixed, tuning).instantiate(q, ap_, ip, gp, n)
        bind_vis(fn, o)
        fn.ensure_all_bound()
        fn.buffer('weights_grid').set(q, np.ones(fn.buffer('weights_grid').shape, np.float32))
        fn.buffer('grid').zero(q)
        dt = _timed(fn, q, args.reps)
        grids[ip.fixed.real_dtype] = fn.buffer('grid')
        print('%-45s %8.3f ms  %6.3f Gvis/s  (%s)' % (name, dt * 1e3, n / dt / 1e9, fn.last_variant))

    for name, ip in (('f64 degridder auto', ip64), ('f32 degridder (auto)', ip32)):
        dg = grid.DegridderTemplate(ctx, ip.fixed, gp.fixed).instantiate(q, ap_, ip, gp, n)
        bind_vis(dg, obs)
        dg.bind(grid=grids[ip.fixed.real_dtype],
                weights=accel.DeviceArray(ctx, (n, 1), np.float32,
                                          tensor=torch.ones((n, 1), device=ctx.device)))
        dg.ensure_all_bound()
        dt = _timed(dg, q, args.reps)
        print('%-45s %8.3f ms  %6.3f Gvis/s  (%s)' % (name, dt * 1e3, n / dt / 1e9, dg.last_variant))

    G = obs.pixels
    for dtype in (np.float64, np.float32):
        t = image.GridImageTemplate(ctx, dtype)
        plan = t.make_fft_plan((G, G))
        g = grids[np.dtype(dtype)]
        g2i = t.instantiate_grid_to_image(q, g.shape, ip32.pixel_size, -0.5 * G * ip32.pixel_size, plan)
        g2i.bind(grid=g)
        g2i.ensure_all_bound()
        g2i.buffer('kernel1d').set(q, np.ones(G, dtype))
        i2g = t.instantiate_image_to_grid(q, g.shape, ip32.pixel_size, -0.5 * G * ip32.pixel_size, plan)
        i2g.bind(grid=g, layer=g2i.buffer('layer'), image=g2i.buffer('image'),
                 kernel1d=g2i.buffer('kernel1d'))
        i2g.ensure_all_bound()
        for w in (0.0, 3.0):
            g2i.set_w(w)
            i2g.set_w(w)
            label = 'f64' if dtype == np.float64 else 'f32'
            print('%-45s %8.3f ms' % ('%s grid->image w=%g' % (label, w), _timed(g2i, q, args.reps) * 1e3))
            print('%-45s %8.3f ms' % ('%s image->grid w=%g' % (label, w), _timed(i2g, q, args.reps) * 1e3))


if __name__ == '__main__':
    main()
