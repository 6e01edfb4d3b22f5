"""The cut of a frame into batches and passes (rt_frame_plan, rustracer_amd/csrc/rtx_frame_plan.h), checked without a device at the shapes it was
tuned for - 2^29 paths per pass, which no GPU test can afford. The invariants are what the kernels rely on when they index the workspace; the worked cases were
derived by hand from render_frame's sizing code as it stood before the cut became a function of its own (defaults: pass log2 29, batch log2 19, lead on at 1024 spp)."""
import itertools

import pytest

from rustracer_amd import host

RT_QSHARDS = 8
RT_ERR_INVALID, RT_ERR_OOM = -1, -4
OWNED = [0, 1, 4095, 4096, 2**15 - 1, 2**15, 2**16, 2**19, 2**19 + 1, 2**20, 3840 * 2160]
SPP = [1, 16, 1024, 4096, 16384]
DIMS = [2, 5, 8]
SHRINK = [0, 5, 15]


@pytest.mark.parametrize("dims, shrink", list(itertools.product(DIMS, SHRINK)))
def test_every_cut_tiles_the_pixels_and_stays_inside_the_workspace(dims, shrink):
    for owned, spp in itertools.product(OWNED, SPP):
        p = host.frame_plan(owned, spp, dims, pass_log2=29 - shrink, n_cu=256)
        where = (owned, spp, dims, shrink, {k: v for k, v in p.items() if k != "batches"})
        batches, cap, bp, lead = p["batches"], p["cap"], p["batch_pixels"], p["lead_pixels"]
        # the batches tile [0, owned) exactly once and in order
        at = 0
        for first, pixels, _ in batches:
            assert first == at and pixels >= 1, where
            at += pixels
        assert at == owned, where
        # only the first batch may be the short lead: the others are whole batches, the last one what is left
        assert lead < bp, where
        for i, (_, pixels, _) in enumerate(batches):
            if i == 0:
                assert pixels == (lead if lead else min(bp, owned)), where
            elif i + 1 < len(batches):
                assert pixels == bp, where
            else:
                assert pixels <= bp, where
        assert p["multi_batch"] == (len(batches) > 1), where
        # no pass of any batch holds more paths than the workspace was sized for (a batch's first pass is its largest)
        assert 1 <= p["pass_samples"] <= spp and bp * p["pass_samples"] == cap, where
        for _, pixels, pass_samples in batches:
            assert 1 <= pass_samples <= spp and pixels * pass_samples <= cap, where
        assert cap <= 2**31 - 1, where
        assert p["n_slots"] >= cap and p["shard_cap"] * RT_QSHARDS == p["n_slots"], where
        # <= 16 GiB of sampler tables (2 * dims tables of spp u16 per pixel) per buffer, down to batches of 4096 pixels
        for _, pixels, _ in batches:
            assert pixels <= 4096 or pixels * 2 * dims * spp * 2 <= 16 << 30, where


@pytest.mark.parametrize("owned, spp, pixels, cap, pass_samples", [
    (2**20, 1024, [65536, 524288, 458752], 2**29, 1024),   # the short lead of an eighth of a batch, then whole batches
    (2**15, 4096, [16384, 16384], 2**26, 4096),            # no lead (4096 spp); fits one batch and is cut in two all the same
    (4096, 16, [4096], 65536, 16)])
def test_cuts_worked_by_hand(owned, spp, pixels, cap, pass_samples):
    p = host.frame_plan(owned, spp, 5, n_cu=256)
    assert [b[1] for b in p["batches"]] == pixels
    assert (p["cap"], p["pass_samples"]) == (cap, pass_samples)


def test_more_cuts_worked_by_hand():
    # the queue shards: cap / 8 entries + 256 per block of a shard's 256 + 1 blocks (n_cu * 8 blocks over 8 shards) + 256
    p = host.frame_plan(4096, 16, 5, n_cu=256)
    assert (p["shard_cap"], p["n_slots"], p["multi_batch"], p["lead_pixels"]) == (8192 + 256 * 257 + 256, 8 * (8192 + 256 * 257 + 256), False, 0)
    # a short batch takes more samples per pass, the same paths: 2^29 / 65536 = 8192 -> spp; 2^29 / 458752 = 1170 -> spp
    assert [b[2] for b in host.frame_plan(2**20, 1024, 5)["batches"]] == [1024, 1024, 1024]
    # ... seen at a pass of 2^24 paths: 2^24 / 2^19 = 32 samples per pass, the lead 2^24 / 65536 = 256, the last batch 2^24 // 458752 = 36
    p = host.frame_plan(2**20, 1024, 5, pass_log2=24)
    assert p["batches"] == [(0, 65536, 256), (65536, 524288, 32), (589824, 458752, 36)] and (p["cap"], p["pass_samples"]) == (2**24, 32)
    # a rank that owns no rows: no batch, a workspace of one pixel
    p = host.frame_plan(0, 16, 5)
    assert (p["batches"], p["batch_pixels"], p["pass_samples"], p["cap"], p["multi_batch"]) == ([], 1, 16, 16, False)
    # the lead is off below 2^16 pixels and below 2^27 samples
    assert host.frame_plan(2**16 - 1, 1024, 5)["lead_pixels"] == 0 and host.frame_plan(2**16, 1, 5, lead_on=True)["lead_pixels"] == 0
    assert host.frame_plan(2**16, 2048, 5, lead_on=True)["lead_pixels"] == 2**15 and host.frame_plan(2**16, 2048, 5)["lead_pixels"] == 0
    # 16 GiB of tables: 8 dims x 16384 spp = 512 KiB per pixel -> 2^15 pixels per batch
    assert host.frame_plan(2**20, 16384, 8)["batch_pixels"] == 2**15


def test_a_resident_frame_keeps_the_cut_its_tables_were_laid_out_by():
    p = host.frame_plan(2**20, 1024, 5, pass_log2=24, fixed_cut=(2**18, 0))
    assert [b[1] for b in p["batches"]] == [2**18] * 4 and (p["lead_pixels"], p["pass_samples"], p["cap"]) == (0, 64, 2**24)
    p = host.frame_plan(2**20, 1024, 5, pass_log2=29, fixed_cut=(2**19, 65536))
    assert [b[1] for b in p["batches"]] == [65536, 524288, 458752] and p["cap"] == 2**29


@pytest.mark.parametrize("shrink", [16, 17, 29, 40])
def test_a_pass_below_2_14_paths_is_out_of_memory(shrink):
    with pytest.raises(host.BackendError, match=r"not enough free device memory for the smallest pass \(2\^14 paths\)") as e:
        host.frame_plan(2**20, 1024, 5, pass_log2=29 - shrink)
    assert e.value.code == RT_ERR_OOM


def test_a_pass_of_2_31_paths_is_refused():
    # 2^32 pixels of 8-byte tables: halved once to 16 GiB, 1 sample per pass -> cap = 2^31
    with pytest.raises(host.BackendError, match="pass too large") as e:
        host.frame_plan(2**32, 1, 2, pass_log2=32, batch_log2=32)
    assert e.value.code == RT_ERR_INVALID
