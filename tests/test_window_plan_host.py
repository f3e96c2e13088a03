"""Host test of the launch-plan helpers the window gridder's kernel shares with its host code
(csrc/kimg_window_plan.h): tests/host/window_plan_harness.cpp, compiled for the host, covers every
chunk count 1 .. 100 000 and every multiple of every candidate multiplier up to 10^7 (the multiplier
chosen is coprime to the count), and checks that the plan the device recomputes for a folded stream
covers that stream with the host's workgroups (spans and chunks are multiples of 64, the chunks tile
the stream, the multiplier is coprime to the device's count).  Host and device evaluate ONE set of
`__host__ __device__` functions, so there are no two forms to compare: the harness only confirms that
`window_partition_of` goes through them.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'katsdpimager_amd', 'csrc')
HARNESS = os.path.join(ROOT, 'tests', 'host', 'window_plan_harness.cpp')


def test_window_plan_helpers(tmp_path):
    from katsdpimager_amd import build
    exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(exe), 'hipcc not found (the library itself cannot be built without it)'
    flags = [f for f in build.FLAGS if not f.startswith('--offload-arch') and f not in ('-fPIC', '-munsafe-fp-atomics')]
    out = str(tmp_path / 'window_plan')
    cmd = [exe, '-x', 'hip', '--offload-host-only', '-no-hip-rt'] + flags + ['-I', CSRC, HARNESS, '-o', out]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, ' '.join(cmd) + '\n' + done.stdout
    done = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert done.returncode == 0 and done.stdout.strip() == 'ok', done.stdout
