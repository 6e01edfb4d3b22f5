"""First-hit feature planes across the workers of one process (rt_multi_frame_read(RT_FRAME_FEATURES) through HostScene.progressive_multi(features=True)): two workers on
the one GPU give the single-device frame's planes bit for bit after plain and after adaptive steps - each pixel is taken from its owner's plane, nothing is added -, and a
worker that owns no row is legal. The scene is (b) of tests/test_gpu_features.py. Every figure is printed before it is asserted."""
import numpy as np
import pytest

from test_gpu_features import FLOOR, _median_gap_threshold, _room
from util import bits

pytestmark = pytest.mark.gpu


def _run(fr, multi, thr=None):
    """advance(3), advance(5) and - with a threshold - an adaptive step of 4: the planes after each, and the samples taken."""
    out = []
    for n in (3, 5):
        fr.advance(n)
        out.append(fr.features())
    if thr is not None:
        fr.advance_adaptive(4, thr, FLOOR, min_samples=4)
        out.append(fr.features())
    return out, fr.samples_taken, fr.active_pixels


def test_two_workers_read_the_single_device_planes(gpu_host):
    h = gpu_host.HostScene(_room())
    with h.progressive(pixel_stats=True) as fr:   # the threshold of the adaptive step, from the statistics after 8 samples
        fr.advance(8)
        thr, lo, hi = _median_gap_threshold(*fr.pixel_stats(), FLOOR)
    assert (hi - lo) / hi > 1e-6
    with h.progressive(pixel_stats=True, features=True) as fr:
        single, taken1, active1 = _run(fr, False, thr)
    with h.progressive_multi([0, 0], pixel_stats=True, features=True) as fr:
        multi, taken2, active2 = _run(fr, True, thr)
        state = fr.state_bytes
    d = [int((bits(a) != bits(b)).sum()) for a, b in zip(single, multi)]
    print(f"\nMULTI FEATURES two workers on one GPU, after 3, 8 samples and an adaptive step of 4 at threshold {thr:.6g}: plane words that differ from the single-device frame's {d}; "
          f"samples taken {taken1} / {taken2}, active pixels {active1} / {active2}; coverage spans [{multi[-1][..., 7].min():.3f}, {multi[-1][..., 7].max():.3f}]")
    assert d == [0, 0, 0]
    assert taken1 == taken2 and active1 == active2 and 0 < active1 < 32 * 32
    assert multi[0][..., :3].any() and multi[0][..., 7].min() < 1.0 and multi[0][..., 7].max() == 1.0
    assert state >= 32 * 32 * 64
    with h.progressive_multi([0, 0], pixel_stats=True) as fr:   # no flag: refused, with the function's name
        fr.advance(2)
        with pytest.raises(gpu_host.BackendError) as e:
            fr.features()
        print(f"  read without the flag refused: {e.value}")
        assert "RT_FLAG_FRAME_FEATURES" in str(e.value) and "rt_multi_frame_read" in str(e.value)


def test_a_worker_that_owns_no_row_is_legal(gpu_host):
    """32 x 8 pixels are two bands of four rows: the third of three workers owns none."""
    d = _room()
    d.film.xres, d.film.yres = 32, 8
    h = gpu_host.HostScene(d)
    with h.progressive(features=True) as fr:
        fr.advance(16)
        single = fr.features()
    with h.progressive_multi([0, 0, 0], features=True) as fr:
        total, per = fr.advance(16)
        multi = fr.features()
    differ = int((bits(single) != bits(multi)).sum())
    print(f"\nMULTI FEATURES three workers, two bands: camera rays per worker {[p['camera_rays'] for p in per]}; plane words that differ from the single-device frame's {differ}")
    assert [p["camera_rays"] for p in per] == [32 * 4 * 16, 32 * 4 * 16, 0] and differ == 0 and single[..., :3].any()
