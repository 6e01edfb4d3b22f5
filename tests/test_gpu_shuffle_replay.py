"""The shuffle replay kernels on partner rows of the caller's (rt_sampler_replay): the parallel replay (k_sampler_shuffle_par, kernel 1) against the chain kernel
(k_sampler_shuffle, kernel 0) and against the sequential swap loop in Python, bit for bit, on random rows and on the rows no random stream produces - and the
segmented sampler's tables against the in-order kernel's on pixel ranges that leave the draws kernel and the replay ragged last workgroups."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPPS = (64, 128, 256, 512, 1024)         # E = 1, 2, 4, 8, 16
CHAINS = (1, 15, 16, 17, 33)             # workgroups of 16 chains: ragged, full, full + 1, two full + 1
RANGES = ((8900, 70), (0, 1), (0, 255), (0, 257), (5, 777))  # pixel 8933 holds a retry at 1024 spp


def sequential(o):
    a = list(range(len(o)))
    for i, p in enumerate(o):
        a[i], a[p] = a[p], a[i]
    return a


def rows_for(spp, n):
    """n partner rows, the kinds in turn: random; all self-swaps; every step to the last position (64 lanes on one word); o_i = min(i + 1, N - 1) (the longest pointer
    chain); one target written from every 64-step instruction (two lanes of each, random elsewhere)."""
    rng = np.random.default_rng(spp * 100 + n)
    idx = np.arange(spp)
    out = []
    for c in range(n):
        kind = c % 5 if n > 1 else 4
        rnd = idx + (rng.random(spp) * (spp - idx)).astype(np.int64)
        if kind == 0:
            o = rnd
        elif kind == 1:
            o = idx.copy()
        elif kind == 2:
            o = np.full(spp, spp - 1)
        elif kind == 3:
            o = np.minimum(idx + 1, spp - 1)
        else:
            o = rnd
            for m in range(spp // 64):
                o[64 * m + 3] = spp - 1
                o[64 * m + 40] = spp - 1
        out.append(o)
    o = np.array(out, np.uint16)
    assert np.all(o >= idx) and np.all(o < spp)
    return o


@pytest.fixture(scope="module")
def cases():
    """{(spp, n): (partners, the sequential loop's permutations)}, computed once"""
    out = {}
    for spp in SPPS:
        for n in CHAINS:
            o = rows_for(spp, n)
            out[spp, n] = (o, np.array([sequential(r.tolist()) for r in o], np.uint16))
    return out


@pytest.mark.parametrize("spp", SPPS)
def test_parallel_replay_equals_the_chain_kernel_and_the_swap_loop(gpu_host, cases, spp):
    for n in CHAINS:
        o, want = cases[spp, n]
        par = gpu_host.sampler_replay(o, kernel=1)
        chain = gpu_host.sampler_replay(o, kernel=0)
        assert np.array_equal(chain, want), (spp, n, np.argwhere(chain != want)[:4].tolist())
        assert np.array_equal(par, want), (spp, n, np.argwhere(par != want)[:4].tolist())


def test_every_wave_on_the_sequential_branch_gives_the_same_permutations(gpu_host, cases, capfd):
    os.environ["RTX_K0_FORCE_RESORT"] = "1"
    os.environ["RTX_K0_REPORT"] = "1"
    try:
        for spp in SPPS:
            for n in CHAINS:
                o, want = cases[spp, n]
                capfd.readouterr()
                par = gpu_host.sampler_replay(o, kernel=1)
                m = re.search(r"k_sampler_shuffle_par: (\d+) wave", capfd.readouterr().err)
                assert m and int(m.group(1)) == n, (spp, n, m and m.group(0))   # one wave pass per chain, every one of them on the branch
                assert np.array_equal(par, want), (spp, n)
    finally:
        del os.environ["RTX_K0_FORCE_RESORT"]
        del os.environ["RTX_K0_REPORT"]


def test_no_wave_takes_the_sequential_branch_unforced(gpu_host, cases, capfd):
    os.environ["RTX_K0_REPORT"] = "1"
    try:
        for spp in SPPS:
            capfd.readouterr()
            gpu_host.sampler_replay(cases[spp, 33][0], kernel=1)
            assert "k_sampler_shuffle_par: 0 wave(s) re-sorted" in capfd.readouterr().err, spp
    finally:
        del os.environ["RTX_K0_REPORT"]


def test_replay_refuses_partners_below_their_step(gpu_host):
    o = np.tile(np.arange(64, dtype=np.uint16), (2, 1))
    o[1, 9] = 8
    with pytest.raises(gpu_host.BackendError):
        gpu_host.sampler_replay(o, kernel=1)
    with pytest.raises(gpu_host.BackendError):
        gpu_host.sampler_replay(np.zeros((1, 32), np.uint16) + 31, kernel=1)   # below the parallel replay's 64


@pytest.mark.parametrize("p0, n", RANGES)
def test_segmented_tables_equal_the_in_order_kernel_at_1024_spp(gpu_host, p0, n):
    a = gpu_host.sampler_tables(1024, 4, p0, n)
    b = gpu_host.sampler_tables(1024, 4, p0, n, plain=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from rustracer_amd import host
for spp in (64, 256):
    for p0, n in %r:
        a = host.sampler_tables(spp, 4, p0, n)
        b = host.sampler_tables(spp, 4, p0, n, plain=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (spp, p0, n)
print("tables equal")
"""


def test_segmented_tables_equal_the_in_order_kernel_with_the_parallel_replay_forced(gpu_host):
    """RTX_K0_PARALLEL is read once per process: a child with the knob set builds the tables of 64 and 256 spp through k_sampler_shuffle_par<1> / <4>."""
    env = dict(os.environ, RTX_K0_PARALLEL="1", RTX_K0_REPORT="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, RANGES)], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tables equal" in r.stdout
    lines = re.findall(r"k_sampler_shuffle_par: (\d+) wave", r.stderr)
    assert lines and all(int(x) == 0 for x in lines), r.stderr[-1000:]   # the parallel kernel ran, no wave left the parallel path
