"""CPU: the host reference of the device noise stream (tests/noise_ref.py) against known answers, against a second
implementation of Philox4x32-10 that ships with PyTorch, and against the statistics a standard normal stream must
have.  The GPU comparison (test_gpu_noise_stream.py) rests on these."""
import os
import subprocess

import numpy as np
import pytest

import noise_ref as R

S = 42100          # seed of the statistical tests (the benchmark's)
ROW = 498          # 3 * 166: one row of the stream
N_STAT = 20_000 * ROW


def hexwords(w):
    return " ".join(f"{int(np.asarray(x).reshape(-1)[0]):08x}" for x in w)


KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert hexwords(R.philox4x32_10(*ctr, *key)) == want


def test_high_words_of_counter_stream_and_key_are_taken():
    assert hexwords(R.words(2**64 - 1, 1, 2**35 + 7)) == "da2abbe7 68b5735e ecaaee0f 26d5f7d2"
    base = hexwords(R.words(2**64 - 1, 1, 2**35 + 7))
    # every one of the six input words matters
    for seed, stream, q in [(2**32 - 1, 1, 2**35 + 7), (2**64 - 2, 1, 2**35 + 7), (2**64 - 1, 0, 2**35 + 7),
                            (2**64 - 1, 1 + 2**32, 2**35 + 7), (2**64 - 1, 1, 7), (2**64 - 1, 1, 2**35 + 6)]:
        assert hexwords(R.words(seed, stream, q)) != base
    assert hexwords(R.words(-1, 1, 2**35 + 7)) == base  # seeds are taken mod 2^64


_SECOND_SOURCE = r"""
#include <ATen/core/PhiloxRNGEngine.h>
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  // argv: counter (q, stream) and key (seed) as 64-bit words; prints the four output words of that counter
  for (int i = 1; i + 2 < argc; i += 3) {
    const uint64_t q = strtoull(argv[i], nullptr, 0), stream = strtoull(argv[i + 1], nullptr, 0);
    const uint64_t seed = strtoull(argv[i + 2], nullptr, 0);
    at::philox_engine eng(seed, stream, 0);
    eng.set_offset(q);
    const uint32_t a = eng(), b = eng(), c = eng(), d = eng();
    std::printf("%08x %08x %08x %08x\n", a, b, c, d);
  }
  return 0;
}
"""


def test_words_agree_with_the_philox_engine_of_pytorch(tmp_path):
    """A second source for the known answers and for the placement of (quad, stream, seed) in counter and key:
    ATen/core/PhiloxRNGEngine.h (header only, host compilable), built here with the host compiler and asked for the
    same counters.  Nothing of it is kept."""
    import shutil

    import torch

    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    assert os.path.exists(os.path.join(inc, "ATen", "core", "PhiloxRNGEngine.h")), "PyTorch ships no PhiloxRNGEngine.h"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "philox_second.cpp", tmp_path / "philox_second"
    src.write_text(_SECOND_SOURCE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", inc, str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True, timeout=300)
    full = 2**64 - 1
    cases = [(0, 0, 0), (full, full, full),
             (0x85A308D3243F6A88, 0x0370734413198A2E, 0x299F31D0A4093822),  # the third known answer
             (2**35 + 7, 1, full), (12345, 0, S), (2**33 + 1, 1, R.call_seed(S, 2))]
    args = [hex(v) for case in cases for v in case]
    got = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    for (q, stream, seed), line in zip(cases, got):
        assert hexwords(R.words(seed, stream, q)) == line.strip(), (q, stream, seed)
    assert got[0].strip() == KNOWN[0][2] and got[1].strip() == KNOWN[1][2] and got[2].strip() == KNOWN[2][2]
    assert got[3].strip() == "da2abbe7 68b5735e ecaaee0f 26d5f7d2"


def test_normal_follows_the_contract_on_one_quad():
    """Words -> uniforms -> Box-Muller, spelled out with Python's math module on one quad."""
    import math

    seed, stream, q = 42100, 1, 2**33 + 5
    w = [int(x) for x in R.words(seed, stream, q)]
    want = []
    for h in (0, 1):
        u1, u2 = (w[2 * h] + 0.5) / 2**32, (w[2 * h + 1] + 0.5) / 2**32
        rad, angle = math.sqrt(-2.0 * math.log(u1)), 6.283185307179586 * u2
        want += [rad * math.cos(angle), rad * math.sin(angle)]
    got = R.normal(seed, stream, 4 * q + np.arange(4))
    assert np.all(np.abs(got - np.array(want)) <= 8 * R.U * np.abs(got))  # (libm in float64 against longdouble)
    assert np.array_equal(got, R.normal_range(seed, stream, 4 * q, 4))


def test_range_form_equals_the_elementwise_form():
    rng = np.random.default_rng(1)
    for g0, n in [(0, 1), (1, 1), (2, 1), (3, 1), (3, 2), (5, 11), (2**40 + 1, 9), (2**34 - 2, 6)]:
        assert np.array_equal(R.normal_range(7, 1, g0, n), R.normal(7, 1, g0 + np.arange(n)))
    g = rng.integers(0, 2**45, 500)
    one_by_one = np.array([R.normal_range(2**40 + 3, 0, int(x), 1)[0] for x in g])
    assert np.array_equal(R.normal(2**40 + 3, 0, g), one_by_one)
    # the float64 evaluation sits within a few u of the extended one (what the statistical tests below use)
    a, b = R.normal_range(S, 0, 0, 100_000), R.normal_range(S, 0, 0, 100_000, extended=False)
    assert np.max(np.abs(a - b) / np.abs(a)) < 8 * R.U


def test_every_mutation_changes_the_reference():
    """The mutated references (the GPU sensitivity test) differ from the true one somewhere."""
    g0 = (2**33) * 150  # a flat index whose quad needs the high counter word
    seed = 2**64 - 1
    z = R.normal_range(seed, 1, g0, 64)
    for m in R.MUTATIONS:
        if m == "call_seed_not_advanced":
            assert R.call_seed(seed, 1, m) != R.call_seed(seed, 1) and R.call_seed(seed, 0, m) == R.call_seed(seed, 0)
            continue
        zm = R.normal_range(seed, 1, g0, 64, mutation=m)
        assert not np.array_equal(zm, z), m
        assert np.array_equal(zm, R.normal(seed, 1, g0 + np.arange(64), mutation=m), equal_nan=True), m


def test_call_seed_wraps():
    assert R.call_seed(5, 0) == 5 and R.call_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert R.call_seed(2**64 - 3, 1) == 0x9E3779B97F4A7C15 - 3
    assert R.call_seed(2**64 - 3, 2) == (2 * 0x9E3779B97F4A7C15 - 3) - 2**64


def test_synth_and_site_references():
    out, z = R.synth_normal_ref(3, 9, np.float64, 11, 2, mean=1.0, sigma=3.0, lattice=1.5, with_z=True)
    assert out.shape == z.shape == (3, 9, 3)
    assert np.array_equal(z.reshape(-1), R.normal(11, 0, 2 * 27 + np.arange(81)))
    # 9 sites: side 3 (the smallest cube that holds them); site 5 sits at (2, 1, 0)
    assert np.array_equal(R.lattice_coord(9)[5], [2, 1, 0]) and np.array_equal(R.lattice_coord(28)[27], [3, 2, 1])
    assert np.array_equal(R.lattice_coord(1), [[0, 0, 0]]) and R.lattice_coord(8).max() == 1 and R.lattice_coord(27).max() == 2
    assert np.array_equal(out, 1.0 + 1.5 * R.lattice_coord(9)[None] + 3.0 * z)
    assert R.synth_normal_ref(3, 9, np.float32, 11, 2).dtype == np.float32
    e = R.site_noise_ref(4, 5, np.float64, 11, 3)
    assert e.shape == (4, 5, 3) and np.array_equal(e.reshape(-1), R.normal(11, 1, 3 * 15 + np.arange(60)))
    # a shard is the same frames of the whole
    assert np.array_equal(R.site_noise_ref(7, 5, np.float64, 11, 0)[3:], e)


# ---- the quality of the stream itself ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams():
    """About 1e7 values each, float64 evaluation, fixed seeds: deterministic."""
    draw = lambda seed, stream: R.normal_range(seed, stream, 0, N_STAT, extended=False)  # noqa: E731
    return {"s": draw(S, 0), "s+1": draw(S + 1, 0), "sites": draw(S, 1),
            "call3": draw(R.call_seed(S, 3), 1), "call4": draw(R.call_seed(S, 4), 1)}


def test_stream_moments(streams):
    z = streams["s"]
    n = z.size
    assert np.isfinite(z).all() and np.max(np.abs(z)) <= R.Z_MAX
    scores = {"mean": z.mean() * np.sqrt(n), "variance": (np.mean(z * z) - 1.0) / np.sqrt(2.0 / n),
              "third moment": np.mean(z ** 3) / np.sqrt(15.0 / n), "fourth moment": (np.mean(z ** 4) - 3.0) / np.sqrt(96.0 / n)}
    print(scores)
    for name, score in scores.items():
        assert abs(score) < 5, f"{name}: z-score {score:.2f}"


@pytest.mark.parametrize("name", ["s", "sites"])
def test_stream_autocorrelation(streams, name):
    z = streams[name]
    for lag in (1, 2, 3, 4, 5, 8, 12, ROW):
        score = np.mean(z[:-lag] * z[lag:]) * np.sqrt(z.size - lag)
        print(name, lag, score)
        assert abs(score) < 5, f"lag {lag}: z-score {score:.2f}"


@pytest.mark.parametrize("a,b", [("s", "s+1"), ("s", "sites"), ("call3", "call4"), ("sites", "call3")])
def test_streams_are_uncorrelated(streams, a, b):
    """Seeds s and s + 1 (the benchmark's forces and coordinates), stream words 0 and 1 of one seed, consecutive calls
    of one augmenter: also shifted against each other by a lane, a quad and a row."""
    x, y = streams[a], streams[b]
    for shift in (0, 1, 2, 4, ROW):
        score = np.mean(x[:x.size - shift] * y[shift:]) * np.sqrt(x.size - shift)
        print(a, b, shift, score)
        assert abs(score) < 5, f"{a} x {b} at shift {shift}: z-score {score:.2f}"


@pytest.mark.parametrize("name", ["s", "sites"])
def test_stream_kolmogorov_smirnov(streams, name):
    import torch

    z = np.sort(streams[name])
    n = z.size
    cdf = torch.special.ndtr(torch.from_numpy(z)).numpy()  # the standard normal distribution function
    i = np.arange(1, n + 1)
    d = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n))
    print(name, np.sqrt(n) * d)
    assert np.sqrt(n) * d < 2
