"""The cache of captured graphs (csrc/kimg_graph_cache.h) on the host alone: tests/host/
graph_cache_harness.cpp includes the header as it is, stands in for the HIP runtime with a scripted
fake, and runs the cache through hits, misses, evictions, device take-overs, every failure exit, a
random walk against a model and eight threads.  No GPU is opened.

The harness is built three ways -- plain, with the address and undefined-behaviour sanitizers, and
with the thread sanitizer (the threaded case only) -- as a stand-alone executable; nothing sanitized
is loaded into Python.  It is then built against mutated copies of the header, each with one of the
cache's rules taken out, and has to fail on every one of them (the list cannot rot: a pattern that
no longer matches the header is a failure)."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'katsdpimager_amd', 'csrc')
HEADER = os.path.join(CSRC, 'kimg_graph_cache.h')
HARNESS = os.path.join(ROOT, 'tests', 'host', 'graph_cache_harness.cpp')
ENTRY_POINTS = ['hipStreamBeginCapture', 'hipStreamEndCapture', 'hipGraphInstantiate', 'hipGraphDestroy',
                'hipGraphExecDestroy', 'hipEventCreateWithFlags', 'hipEventDestroy', 'hipEventQuery',
                'hipEventRecord', 'hipGetDevice', 'hipGetLastError', 'hipPeekAtLastError']
CASES = ['hit_and_miss', 'fill_order', 'eviction_rule', 'device_takeover', 'failure_exits', 'release_rule',
         'unqueryable_event', 'not_ready_is_not_an_error', 'model_check', 'threads']

# flavour -> (extra compiler flags, the harness's argument)
FLAVOURS = {
    'plain': ([], 'all'),
    'asan_ubsan': (['-g', '-fno-omit-frame-pointer', '-Xarch_host', '-fsanitize=address,undefined',
                    '-Xarch_host', '-fno-sanitize-recover=undefined'], 'all'),
    'tsan': (['-g', '-Xarch_host', '-fsanitize=thread'], 'threads'),
}

# name -> (text in the header, what replaces it, a case that has to notice)
MUTANTS = {
    'evicts a pinned entry': (
        'if (slots[i].users == 0\n', 'if (true\n', 'eviction_rule'),
    'evicts without asking the event': (
        'hipEventQuery(slots[i].last_use) == hipSuccess', 'true', 'eviction_rule'),
    'keeps the graph after instantiating it': (
        '        (void) hipGraphDestroy(graph);\n        if (e != hipSuccess)', '        if (e != hipSuccess)',
        'fill_order'),
    'gives up without reading the last error': (
        '        (void) hipGetLastError();\n        return nullptr;', '        return nullptr;', 'failure_exits'),
    'compares all bytes but the last': (
        'memcmp(&slots[i].args, &a, sizeof(a))', 'memcmp(&slots[i].args, &a, sizeof(a) - 1)', 'hit_and_miss'),
    'keeps the event of another device': (
        'if (slot->device != device) {', 'if (false) {', 'device_takeover'),
    'leaves the event queries\' error behind': (
        '            if (clean)\n                (void) hipGetLastError();\n', '', 'not_ready_is_not_an_error'),
}


def compiler():
    from katsdpimager_amd import build
    exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(exe):
        pytest.skip('hipcc not found: the host harness of the graph cache cannot be built')
    # the library's own flags, where they apply to host code (no code object, no shared library);
    # host only, and without the HIP runtime: every hip* symbol has to come from the harness
    flags = [f for f in build.FLAGS if not f.startswith('--offload-arch') and f not in ('-fPIC', '-munsafe-fp-atomics')]
    return [exe, '-x', 'hip', '--offload-host-only', '-no-hip-rt'] + flags


def compile_harness(out, extra=(), include=None):
    cmd = compiler() + list(extra)
    if include:
        cmd += ['-I', include]
    cmd += ['-I', CSRC, HARNESS, '-o', out, '-pthread']
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, ' '.join(cmd) + '\n' + done.stdout
    return out


def run_harness(exe, what):
    done = subprocess.run([exe, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return done.returncode, done.stdout


@pytest.fixture(scope='module')
def built(tmp_path_factory):
    """Every build this module needs, made side by side: {flavour or mutant name: executable}."""
    compiler()
    tmp = tmp_path_factory.mktemp('graph_cache')
    header = open(HEADER).read()
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        for name, (flags, _) in FLAVOURS.items():
            jobs[name] = pool.submit(compile_harness, str(tmp / name), flags)
        for i, (name, (old, new, _)) in enumerate(MUTANTS.items()):
            if header.count(old) != 1:
                jobs[name] = None       # (reported by the mutant's own test)
                continue
            where = tmp / ('mutant%d' % i)
            where.mkdir()
            (where / 'kimg_graph_cache.h').write_text(header.replace(old, new))
            jobs[name] = pool.submit(compile_harness, str(where / 'harness'), (), str(where))
    return jobs


def tripped(output):
    return sorted(set(re.findall(r'^FAILED (\w+)<', output, re.M)))


@pytest.mark.parametrize('flavour', list(FLAVOURS))
def test_harness_passes(built, flavour):
    exe = built[flavour].result()
    code, out = run_harness(exe, FLAVOURS[flavour][1])
    print(out)
    assert code == 0, out
    assert not re.search(r'Sanitizer|runtime error', out), out
    ran = set(re.findall(r'^ok (\w+)<(?:4|32)>$', out, re.M))
    assert ran == (set(CASES) if FLAVOURS[flavour][1] == 'all' else {'threads'})
    assert len(re.findall(r'^ok ', out, re.M)) == 2 * len(ran)         # 4 slots and 32


def test_harness_calls_its_own_runtime(built):
    """The fake's entry points are defined in the executable, and the HIP runtime is not linked."""
    exe = built['plain'].result()
    nm = shutil.which('nm')
    assert nm and shutil.which('ldd')
    symbols = subprocess.run([nm, '--defined-only', exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = set(re.findall(r' T (\w+)$', symbols, re.M))
    assert set(ENTRY_POINTS) <= defined, set(ENTRY_POINTS) - defined
    assert any(re.fullmatch(r'_Z\d+kimg_capture_streamv', s) for s in defined)
    undefined = subprocess.run([nm, '--undefined-only', exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not re.search(r'\b(hip|hsa|kimg_)', undefined), undefined
    libs = subprocess.run(['ldd', exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not re.search(r'amdhip|hsa-runtime|libkimg', libs), libs


@pytest.mark.parametrize('mutant', list(MUTANTS))
def test_harness_sees_every_mutant(built, mutant):
    old, new, case = MUTANTS[mutant]
    assert built[mutant] is not None, 'the header no longer holds %r: update the mutant' % old
    code, out = run_harness(built[mutant].result(), 'all')
    print('%s: tripped %s' % (mutant, ', '.join(tripped(out))))
    assert code != 0, out
    assert case in tripped(out), out
