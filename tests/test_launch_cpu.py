"""The launch helpers that need no GPU: csrc/xcd_sched.h (persistent XCD-aware tile schedule, both halves) and csrc/dispatch.h
(runtime value -> template argument), each built into a stand-alone host program and run.  No library load."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'iodine_amd', 'csrc')

XCD_PROGRAM = r'''
#include "xcd_sched.h"
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s: ", #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// every tile of [0, ntiles) exactly once over the blocks of `grid`; xcd order: a block stays inside its XCD's eighth
static void cover(int ntiles, int grid, bool xcd_order)
{
    std::vector<int> seen(ntiles, 0);
    const int per_xcd = (ntiles + 7) / 8;
    for (int b = 0; b < grid; ++b) {
        const XcdSpan s = xcd_span(ntiles, grid, b, xcd_order);
        CHECK(s.stride >= 1, "ntiles %d grid %d b %d stride %d", ntiles, grid, b, s.stride);
        if (s.stride < 1) return;
        for (int t = s.first; t < s.end; t += s.stride) {
            CHECK(t >= 0 && t < ntiles, "ntiles %d grid %d b %d tile %d", ntiles, grid, b, t);
            if (t < 0 || t >= ntiles) return;
            ++seen[t];
            if (xcd_order)
                CHECK(t >= (b & 7) * per_xcd && t < ((b & 7) + 1) * per_xcd, "ntiles %d grid %d b %d tile %d outside its eighth", ntiles, grid, b, t);
        }
    }
    for (int t = 0; t < ntiles; ++t) CHECK(seen[t] == 1, "ntiles %d grid %d order %d: tile %d taken %d times", ntiles, grid, (int)xcd_order, t, seen[t]);
}

int main()
{
    std::vector<int> sizes;
    for (int n = 1; n <= 300; ++n) sizes.push_back(n);
    for (int n : {4096, 14336, 57344}) sizes.push_back(n);
    long cases = 0;
    for (int ntiles : sizes) {
        for (int n_cu : {1, 8, 64, 256, 304})
            for (int bpc : {1, 2, 3, 4}) {
                const int full = iod_xcd_grid(ntiles, bpc, n_cu);
                for (int grid : {full, full < 512 ? full : 512, full < 1024 ? full : 1024}) {       // the caps the callers apply
                    CHECK(grid % 8 == 0 && grid >= 8, "ntiles %d n_cu %d bpc %d grid %d", ntiles, n_cu, bpc, grid);
                    cover(ntiles, grid, true);
                    ++cases;
                }
                const int want = bpc * n_cu / 8 > 1 ? bpc * n_cu / 8 : 1, per = (ntiles + 7) / 8;
                CHECK(full == 8 * (per < want ? per : want), "ntiles %d n_cu %d bpc %d grid %d", ntiles, n_cu, bpc, full);
            }
        for (int grid = 1; grid <= 20; ++grid)
            if (grid % 8 != 0) { cover(ntiles, grid, false); ++cases; }
    }
    printf("%ld cases, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
'''

DISPATCH_PROGRAM = r'''
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorUnknown = 999 };     // stand-in: dispatch.h needs only these names
#include "dispatch.h"
#include <cstdio>
#include <initializer_list>

template <int V> static hipError_t probe(int* got) { *got = V; return V == 5 ? hipErrorUnknown : hipSuccess; }

int main()
{
    int fails = 0, calls = 0, got = -1;
    auto f = [&](auto v) { ++calls; return probe<v>(&got); };
    for (int v : {3, 5, 7}) {
        got = -1; calls = 0;
        const hipError_t e = iod_dispatch<3, 5, 7>(v, f);
        if (got != v || calls != 1 || e != (v == 5 ? hipErrorUnknown : hipSuccess)) { ++fails; fprintf(stderr, "FAIL v %d got %d calls %d e %d\n", v, got, calls, (int)e); }
    }
    for (int v : {-1, 0, 4, 8, 1 << 30}) {                  // unmatched: the error, and f is not called
        got = -1; calls = 0;
        const hipError_t e = iod_dispatch<3, 5, 7>(v, f);
        if (e != hipErrorInvalidValue || calls != 0 || got != -1) { ++fails; fprintf(stderr, "FAIL unmatched %d: e %d calls %d\n", v, (int)e, calls); }
    }
    // nested, as the launchers use it: the inner closure sees both constants
    int a = 0, b = 0;
    const hipError_t e2 = iod_dispatch<64, 32>(32, [&](auto cc) { return iod_dispatch<1, 2, 4, 8>(4, [&](auto np) { a = cc; b = np; return hipSuccess; }); });
    if (e2 != hipSuccess || a != 32 || b != 4) { ++fails; fprintf(stderr, "FAIL nested %d %d\n", a, b); }
    const hipError_t e3 = iod_dispatch<64, 32>(32, [&](auto) { return iod_dispatch<1, 2>(3, [&](auto) { a = -1; return hipSuccess; }); });
    if (e3 != hipErrorInvalidValue || a != 32) { ++fails; fprintf(stderr, "FAIL nested unmatched\n"); }
    for (bool v : {false, true}) {
        int seen = -1;
        const hipError_t e = iod_dispatch_bool(v, [&](auto c) { constexpr bool C = c; seen = C; return hipSuccess; });
        if (e != hipSuccess || seen != (int)v) { ++fails; fprintf(stderr, "FAIL bool %d\n", (int)v); }
    }
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
'''


def _host_compiler():
    for c in ('/opt/rocm/bin/hipcc', shutil.which('hipcc'), shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')):
        if c and os.path.exists(c):
            return c
    return None


def _build_and_run(tmp_path, name, text, extra=()):
    cxx = _host_compiler()
    if not cxx:
        pytest.skip('no C++ compiler installed')
    src, exe = tmp_path / (name + '.cpp'), tmp_path / name
    src.write_text(text)
    # plain host C++: nothing of HIP is on the command line, so the headers must stand alone
    r = subprocess.run([cxx, '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, *extra, str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_xcd_schedule_covers_every_tile_once(tmp_path):
    out = _build_and_run(tmp_path, 'xcd_sched', XCD_PROGRAM)
    assert out.strip().endswith('0 failures'), out


def test_dispatch_reaches_the_matching_constant(tmp_path):
    out = _build_and_run(tmp_path, 'dispatch', DISPATCH_PROGRAM)
    assert out.strip() == '0 failures', out


def test_helpers_under_sanitizers(tmp_path):
    """The same two stand-alone host programs with AddressSanitizer and UBSan (host programs of their own: nothing is preloaded)."""
    san = ('-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g')
    cxx = _host_compiler()
    if not cxx:
        pytest.skip('no C++ compiler installed')
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx, '-x', 'c++', *san, str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('sanitizer runtimes not installed')
    assert _build_and_run(tmp_path, 'xcd_sched_san', XCD_PROGRAM, san).strip().endswith('0 failures')
    assert _build_and_run(tmp_path, 'dispatch_san', DISPATCH_PROGRAM, san).strip() == '0 failures'
