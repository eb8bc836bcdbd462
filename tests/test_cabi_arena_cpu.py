"""tests/cabi_arena.py without a GPU: the layout planner and the byte checker on a numpy buffer standing in for the arena."""
import numpy as np
import pytest

from tests.cabi_arena import ALIGN, DEFAULT_GUARD, ArenaDamage, Region, assert_clean, check_bytes, fill_pattern, plan


def _regions(mis=0):
    return [Region("image", 50 * 37, np.float32, "in", mis), Region("tmp", 2 * 50 * 37 + 1024, np.float32, "scratch", mis),
            Region("band0", 25 * 19, np.float32, "out", mis), Region("band1", 25 * 19, np.float32, "inout", mis),
            Region("scr", 33, np.float64, "scratch", mis, guard_elems=300)]


def _packed():
    bands = [Region("band%d" % k, n, np.float32, "in" if k else "inout") for k, n in enumerate([25 * 19, 25 * 19, 13 * 10, 13 * 10 + 1])]
    return [Region("image", 50 * 37, np.float32, "out", 1), bands, Region("tmp", 5000, np.float32, "scratch")]


def test_default_guard_is_wider_than_a_trash_slot():
    assert DEFAULT_GUARD >= 256 and DEFAULT_GUARD > 1024  # dwt_stream.hpp: 1024-float slots


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_planner_alignment_guards_and_no_overlap(mis):
    flat, total = plan(_regions(mis))
    assert total % ALIGN == 0
    spans = sorted((r.offset, r.offset + r.nbytes, r) for r in flat)
    for lo, hi, r in spans:
        assert (lo - mis * r.dtype.itemsize) % ALIGN == 0, r  # exactly the requested misalignment off a 256-byte boundary
        assert lo % r.dtype.itemsize == 0
        assert hi + r.guard_elems * r.dtype.itemsize <= total, r
        assert lo >= r.guard_elems * r.dtype.itemsize, r
    for (_, hi0, r0), (lo1, _, r1) in zip(spans, spans[1:]):
        # at least the larger of the two guards between neighbours
        assert lo1 - hi0 >= max(r0.guard_elems * r0.dtype.itemsize, r1.guard_elems * r1.dtype.itemsize), (r0, r1)


def test_planner_packed_mode():
    flat, total = plan(_packed())
    by = {r.name: r for r in flat}
    bands = [by["band%d" % k] for k in range(4)]
    assert bands[0].offset % ALIGN == 0
    for a, b in zip(bands, bands[1:]):
        assert b.offset == a.offset + a.nbytes  # back to back, band order
    assert bands[1].offset % 16 != 0  # 475 floats: packing itself misaligns the next band
    g = DEFAULT_GUARD * 4
    assert bands[0].offset - (by["image"].offset + by["image"].nbytes) >= g
    assert by["tmp"].offset - (bands[3].offset + bands[3].nbytes) >= g
    assert (by["image"].offset - 4) % ALIGN == 0
    assert total >= by["tmp"].offset + by["tmp"].nbytes + g


def test_fill_pattern_is_position_dependent_and_finite():
    p = fill_pattern(1 << 16)
    w = p.view(np.uint32)
    assert np.unique(w).size > 0.99 * w.size
    assert np.isfinite(p.view(np.float32)).all() and np.isfinite(p.view(np.float64)).all()
    # any two aligned 1 KiB windows differ: a guard copied over another guard is a change
    blocks = p.reshape(-1, 1024)
    assert np.unique(blocks, axis=0).shape[0] == blocks.shape[0]


def _arena(regions):
    flat, total = plan(regions)
    return flat, {r.name: r for r in flat}, fill_pattern(total)


def _one(flat, before, after):
    reps = check_bytes(flat, before, after)
    with pytest.raises(ArenaDamage):
        assert_clean(flat, before, after, "ctx")
    return reps


def test_checker_one_byte_directly_behind_a_payload():
    flat, by, before = _arena(_regions(1))
    after = before.copy()
    r = by["band0"]
    after[r.offset + r.nbytes] ^= 0x10
    reps = _one(flat, before, after)
    assert reps == [dict(region="band0", side="behind", first=0, last=0, bytes=1)]
    with pytest.raises(ArenaDamage, match=r"band0 +BEHIND the payload, bytes \+0 \.\. \+0"):
        assert_clean(flat, before, after)


def test_checker_write_directly_in_front_of_a_payload():
    flat, by, before = _arena(_regions(1))
    after = before.copy()
    r = by["tmp"]
    after[r.offset - 4:r.offset] ^= 0xFF
    reps = _one(flat, before, after)
    assert reps == [dict(region="tmp", side="front", first=-4, last=-1, bytes=4)]


def test_checker_write_in_the_middle_of_a_guard_and_at_the_arena_ends():
    flat, by, before = _arena(_regions())
    after = before.copy()
    r = by["band1"]
    after[r.offset + r.nbytes + 2000:r.offset + r.nbytes + 2016] = 0
    reps = _one(flat, before, after)
    assert len(reps) == 1 and reps[0]["region"] == "band1" and reps[0]["side"] == "behind" and reps[0]["first"] == 2000
    for pos, name, side in ((0, "image", "front"), (before.size - 1, "scr", "behind")):
        after = before.copy()
        after[pos] ^= 1
        reps = _one(flat, before, after)
        assert len(reps) == 1 and (reps[0]["region"], reps[0]["side"]) == (name, side)


def test_checker_changed_in_payload():
    flat, by, before = _arena(_regions(2))
    after = before.copy()
    r = by["image"]
    after[r.offset + 40] ^= 1
    after[r.offset + r.nbytes - 1] ^= 1
    reps = _one(flat, before, after)
    assert reps == [dict(region="image", side="payload(in)", first=40, last=r.nbytes - 1, bytes=2)]


def test_checker_one_guard_copied_over_another():
    flat, by, before = _arena(_regions())
    after = before.copy()
    a, b = by["band0"], by["band1"]
    g = 1024
    after[b.offset - g:b.offset] = before[a.offset - g:a.offset]  # band0's front guard over band1's
    reps = _one(flat, before, after)
    assert len(reps) == 1 and reps[0]["region"] == "band1" and reps[0]["side"] == "front" and reps[0]["bytes"] > 0.75 * g  # (one byte in four carries the forced exponent: few distinct values)


def test_checker_packed_neighbour_and_end_guards():
    flat, by, before = _arena(_packed())
    after = before.copy()
    b1 = by["band1"]
    after[b1.offset + b1.nbytes:b1.offset + b1.nbytes + 4] ^= 0x55  # band1 overruns by one float: that is band2 (`in`)
    reps = _one(flat, before, after)
    assert reps == [dict(region="band2", side="payload(in)", first=0, last=3, bytes=4)]
    after = before.copy()
    b3 = by["band3"]
    after[b3.offset + b3.nbytes] ^= 1
    assert _one(flat, before, after) == [dict(region="band3", side="behind", first=0, last=0, bytes=1)]


def test_checker_passes_when_only_out_inout_and_scratch_change():
    flat, by, before = _arena(_regions(1))
    after = before.copy()
    for name in ("tmp", "band0", "band1", "scr"):
        r = by[name]
        after[r.offset:r.offset + r.nbytes] ^= 0xA5
    assert check_bytes(flat, before, after) == []
    assert_clean(flat, before, after)
