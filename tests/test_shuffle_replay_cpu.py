"""The parallel replay of the Fisher-Yates chain as k_sampler_shuffle_par does it: one returning max per step on a zeroed word array, issued in
ascending step order, names the step's predecessor at its target (the old value) and leaves every position's last writer behind; L, R by pointer jumping and perm
follow. Held here, as a Python model, to the sequential swap loop; a second model serves the lanes of one 64-step instruction in descending order and must be caught by
the kernel's check. The built kernels' LDS and scratch are read from the library."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 64, 1024)
WAVE = 64


def sequential(o):
    a = list(range(len(o)))
    for i, p in enumerate(o):
        a[i], a[p] = a[p], a[i]
    return a


def one_atomic_replay(o, descending=False):
    """(perm or None, tripped groups, jumping rounds). Steps i = 64 m + lane go out one instruction (64 steps) after the other; inside an instruction the lanes are
    served in ascending order, or - descending=True - the other way round. tripped: the (instruction, target) pairs whose check failed; perm is None if any did."""
    n = len(o)
    last, pred, tripped = [0] * n, [0] * n, set()
    for m0 in range(0, n, WAVE):
        lanes = range(m0, min(m0 + WAVE, n))
        for i in (reversed(lanes) if descending else lanes):
            old = last[o[i]]
            last[o[i]] = max(old, i + 1)
            pred[i] = old
            if old > i:  # a larger step was served first: never in ascending order, where old - 1 is an earlier step
                tripped.add((m0 // WAVE, o[i]))
    if tripped:
        return None, tripped, 0
    r = []
    for p in range(n):
        lw = last[p]
        if lw == 0:
            r.append(p)                              # nobody writes p: its own root
        elif lw - 1 < p:
            r.append(lw - 1)                         # the last writer below p
        else:
            assert lw - 1 == p                       # o_i >= i: the self-swap, always the last writer of p
            r.append(pred[p] - 1 if pred[p] else p)  # the writer before it
    rounds = 0
    while True:
        rounds += 1
        nxt = [r[r[p]] for p in range(n)]
        changed = nxt != r
        r = nxt
        if not changed:
            break
    return [r[pred[i] - 1] if pred[i] else o[i] for i in range(n)], tripped, rounds


def random_row(n, rng):
    return [i + int(rng.integers(0, n - i)) for i in range(n)]


def adversarial_rows(n):
    return dict(self_swaps=list(range(n)), all_to_last=[n - 1] * n, next=[min(i + 1, n - 1) for i in range(n)])


@pytest.mark.parametrize("n", SIZES)
def test_one_atomic_replay_is_the_sequential_swap_loop(n):
    rng = np.random.default_rng(1000 + n)
    rows = [random_row(n, rng) for _ in range(40 if n < 1024 else 6)] + list(adversarial_rows(n).values())
    for o in rows:
        perm, tripped, rounds = one_atomic_replay(o)
        assert not tripped
        assert perm == sequential(o), o[:16]
        assert rounds <= max(1, int(np.ceil(np.log2(n)))) + 1  # chain lengths halve per round; one more round sees nothing change


def test_the_longest_pointer_chain_takes_eleven_rounds_at_1024():
    _, _, rounds = one_atomic_replay(adversarial_rows(1024)["next"])
    assert rounds == 11


@pytest.mark.parametrize("n", SIZES)
def test_descending_service_trips_the_check_for_every_group_inside_an_instruction(n):
    rng = np.random.default_rng(2000 + n)
    rows = [random_row(n, rng) for _ in range(40 if n < 1024 else 6)] + list(adversarial_rows(n).values())
    some = False
    for o in rows:
        groups = {}
        for i, p in enumerate(o):
            groups.setdefault((i // WAVE, p), []).append(i)
        want = {k for k, w in groups.items() if len(w) >= 2}
        perm, tripped, _ = one_atomic_replay(o, descending=True)
        assert tripped == want
        assert (perm is None) == bool(want)
        if not want:
            assert perm == sequential(o)  # no two lanes of one instruction shared a word: the order inside it cannot matter
        some |= bool(want)
    assert some or n == 1


@pytest.fixture(scope="module")
def resources(host):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_budget
    finally:
        sys.path.pop(0)
    return kernel_budget.kernel_resources(host.HIP_LIB)


def test_the_replay_at_1024_spp_fits_three_workgroups_per_cu(resources):
    r = resources["rtx::k_sampler_shuffle_par<16>"]
    print(r)
    assert r["lds"] <= 54613, r  # 160 KiB / 3
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0, r


def test_the_draws_kernel_keeps_out_of_scratch(resources):
    import re
    r, pm = resources["rtx::k_sampler_draws<true>"], resources["rtx::k_sampler_draws<false>"]  # chain-major and pixel-minor partner rows
    print(r, pm)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0, r
    assert pm["scratch"] == 0 and pm["vgpr_spills"] == 0 and pm["lds"] == 0, pm
    # its stage is dynamic LDS, asked for by the chain-major launches only (RT_DRAWS_STAGE_BYTES, rtx_kernels.h): static and dynamic together
    src = open(os.path.join(ROOT, "rustracer_amd", "csrc", "rtx_kernels.h")).read()
    stage = int(re.search(r"#define RT_DRAWS_STAGE_BYTES (\d+)u", src).group(1))
    launch = open(os.path.join(ROOT, "rustracer_amd", "csrc", "rtx_hip.hip")).read()
    assert re.search(r"k_sampler_draws<true>,[^;]*\bRT_DRAWS_STAGE_BYTES\b", launch)  # the chain-major launch asks for the stage by that name
    assert stage >= 4 * 64 * 128 and r["lds"] + stage <= 40960, (r, stage)
