"""The node pipeline's scratch plan with 32-byte hit records (csrc/launch.h SKR_REC_BYTES, skr_records_bytes; csrc/render_nodes.hip
plan_for) — no GPU.  The plan is asked of the library's own arithmetic through
skr_nodes_plan_map (internal), the header rows through skr_trace_header_map: a level's record table is 64 regions x cap x 32 bytes, no
two tables of a plan overlap for 1 .. 64 children per node, and a level whose last block of 64 nodes is partial still fits the rows
and the regions the plan gave it.  A launch of which not even one 16x16 block fits the budget with 32-byte records is planned with 16-byte
ones, as it was before there were wide records (plan_bands)."""
import ctypes as C

import pytest

import skele_raytracer_amd as skr

REGIONS, SHARDS, LEVELS_MAX = 64, 4096, 33


def plan(width, rows, N, depth, flat, budget_mb=0, nblk=0):
    fn = skr.lib().skr_nodes_plan_map
    fn.argtypes = [C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    out = (C.c_uint64 * (16 + 8 * LEVELS_MAX))()
    if not fn(width, rows, N, depth, int(flat), budget_mb, nblk, out):
        return None
    names = ("levels", "band_nblk", "total", "banded", "off_ctr", "ctr_bytes", "off_cls", "off_sums", "off_girow", "rec_bytes")
    pl = dict(zip(names, (int(v) for v in out[:10])))
    keys = ("nodes_max", "cap", "off_nodes", "off_shade", "off_recs", "off_res", "off_ixh", "recs_bytes")
    pl["level"] = [dict(zip(keys, (int(v) for v in out[16 + 8 * L:24 + 8 * L]))) for L in range(pl["levels"])]
    return pl


def header_map(nodes, N):
    fn = skr.lib().skr_trace_header_map
    fn.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    fn.restype = C.c_uint32
    out = (C.c_uint64 * 3)()
    fn(nodes, N, out, None, None)
    return dict(rows_used=int(out[0]), rows_alloc=int(out[1]), cap=int(out[2]))


def tables(pl, N):
    """(offset, bytes, name) of every table of the plan, sized as the kernels use them."""
    t = [(pl["off_ctr"], pl["ctr_bytes"], "counters")]
    levels = pl["levels"]
    for L, lv in enumerate(pl["level"]):
        n = lv["nodes_max"]
        if L > 0:
            t.append((lv["off_recs"], lv["recs_bytes"], "records %d" % L))
            t.append((lv["off_res"], n * 12 + 16, "results %d" % L))
        if L < levels - 1 or levels == 1:
            t.append((lv["off_nodes"], n * 32, "geometry rows %d" % L))
            t.append((lv["off_shade"], n * 32, "shading rows %d" % L))
        if L < levels - 1:
            t.append((lv["off_ixh"], header_map(n, N)["rows_alloc"] * 48, "headers %d" % L))
    px = pl["band_nblk"] * 256
    t.append((pl["off_cls"], px, "classes"))
    t.append((pl["off_sums"], SHARDS * 4 * 8, "sums"))
    t.append((pl["off_girow"], px * 4, "GI rows"))
    return t


def test_a_record_is_32_bytes():
    assert plan(64, 36, 4, 3, False, nblk=1)["rec_bytes"] == 32


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_record_tables_are_cap_times_32_bytes_and_no_tables_overlap(depth, flat):
    for N in range(1, 65):
        for nblk in (1, 3):
            pl = plan(64, 36, N, depth, flat, nblk=nblk)
            assert pl is not None, (N, depth, flat, nblk)
            assert pl["levels"] == depth - 1 + (1 if flat else 0) and pl["band_nblk"] == nblk
            assert pl["level"][0]["nodes_max"] == nblk * 256
            for L in range(1, pl["levels"]):
                lv, up = pl["level"][L], pl["level"][L - 1]
                assert lv["cap"] == header_map(up["nodes_max"], N)["cap"], (N, L)
                assert lv["nodes_max"] == REGIONS * lv["cap"]
                assert lv["recs_bytes"] == REGIONS * lv["cap"] * 32, (N, L, lv)  # the size function: cap x 32 bytes per region
                # a level of nodes whose last block of 64 is partial uses no more rows and no more of a region than the full level
                part = header_map(up["nodes_max"] - 37, N)
                assert part["rows_used"] + 4 <= header_map(up["nodes_max"], N)["rows_alloc"]
                assert part["cap"] <= lv["cap"] and (part["rows_used"] + REGIONS - 1) // REGIONS * 128 <= lv["cap"]
            t = sorted(tables(pl, N))
            for (o, b, name), (o2, _, name2) in zip(t, t[1:]):
                assert o % 256 == 0 and b > 0, (N, name, o, b)
                assert o + b <= o2, "N=%d: %s [%d, %d) runs into %s at %d" % (N, name, o, o + b, name2, o2)
            assert t[-1][0] + t[-1][1] <= pl["total"]
            assert [n for _, _, n in t[-3:]] == ["classes", "sums", "GI rows"]  # the kept stage, behind every table that grows with the band
            assert pl["off_cls"] == pl["level"][0]["off_nodes"] + pl["banded"]  # what grows with the band ends where the kept stage begins


def narrow_banded(pl):
    """The banded bytes the same plan would have with 16-byte records (tables on 256-byte boundaries)."""
    up = lambda v: (v + 255) & ~255
    return pl["banded"] - sum(up(lv["nodes_max"] * 32) - up(lv["nodes_max"] * 16) for lv in pl["level"][1:])


def test_a_budget_that_held_16_byte_records_in_one_band_needs_two():
    """64x36, --gillum 16, depth 3 on the persistent schedule: 12 blocks are 48 node blocks x 8 header rows = 384 rows, six per region, so a
    region holds 768 records and the level 49 152: 1.5 MiB of 32-byte records where 16-byte ones took 0.75 MiB.  With the result table
    (0.56 MiB), the level-0 rows and the headers the band's tables are 2.27 MiB against 1.52 MiB: a budget of 2 MiB held the frame in one
    band and now cuts it in two (tests/test_wide_records_gpu.py renders it)."""
    whole = plan(64, 36, 16, 3, False, nblk=12)
    assert whole["level"][1]["cap"] == 768 and whole["level"][1]["recs_bytes"] == 49152 * 32
    budget = 2 << 20
    assert narrow_banded(whole) <= budget < whole["banded"], (narrow_banded(whole), whole["banded"])
    pl = plan(64, 36, 16, 3, False, budget_mb=2)
    assert pl["rec_bytes"] == 32 and pl["band_nblk"] == 8 and pl["banded"] <= budget  # two block rows, then the third: two bands
    assert plan(64, 36, 16, 3, False)["band_nblk"] == 12  # (the default budget: one band)


def narrow_budget(w, h, N, depth, flat):
    """The smallest budget in MiB under which the launch is planned with 16-byte records: one block's tables fit it with them and not
    with 32-byte ones.  None: no whole number of MiB lies between the two."""
    for mb in range(1, 65):
        pl = plan(w, h, N, depth, flat, budget_mb=mb)
        if pl is not None:
            return mb if pl["rec_bytes"] == 16 else None
    return None


def test_a_launch_whose_single_block_needs_16_byte_records_gets_them():
    """16x36, --gillum 97 under 1 MiB (tests/test_trace_by_node_gpu.py test_three_bands): one block's 32 768 records and results are 1.4 MiB
    with 32-byte records and 0.9 MiB with 16-byte ones.  The launch was planned before there were wide records and still is, with the
    16-byte form, one block per band; under 2 MiB a block fits with wide records, two blocks (2.4 MiB) do not.  Where not even 16-byte
    records fit there is no plan, as before."""
    pl = plan(16, 36, 97, 3, False, budget_mb=1)
    assert pl is not None and pl["rec_bytes"] == 16 and pl["band_nblk"] == 1 and pl["banded"] <= 1 << 20
    assert pl["level"][1]["nodes_max"] == 32768 and pl["level"][1]["recs_bytes"] == 32768 * 16
    assert plan(16, 36, 97, 3, False, nblk=1)["banded"] > 1 << 20  # (the same block with wide records)
    assert narrow_budget(16, 36, 97, 3, False) == 1
    pl = plan(16, 36, 97, 3, False, budget_mb=2)
    assert pl["rec_bytes"] == 32 and pl["band_nblk"] == 1
    assert plan(16, 36, 97, 3, False, nblk=2)["banded"] > 2 << 20
    assert plan(16, 36, 256, 3, False, budget_mb=1) is None  # 65 536 records: 1.75 MiB even at 16 bytes


def test_the_record_form_costs_bands_never_a_plan():
    """For every budget from 1 to 16 MiB and a spread of N: wide records wherever one block fits with them — in as many bands as that
    takes — and a plan wherever 16-byte records have one."""
    for N in (1, 4, 16, 33, 64, 97):
        for depth, flat in ((3, False), (3, True), (4, False)):
            one_wide = plan(64, 36, N, depth, flat, nblk=1)
            for mb in range(1, 17):
                pl = plan(64, 36, N, depth, flat, budget_mb=mb)
                fits_wide = one_wide is not None and one_wide["banded"] <= mb << 20
                if fits_wide:
                    assert pl is not None and pl["rec_bytes"] == 32 and pl["banded"] <= mb << 20, (N, depth, flat, mb)
                elif pl is not None:
                    assert pl["rec_bytes"] == 16 and pl["band_nblk"] >= 1 and pl["banded"] <= mb << 20, (N, depth, flat, mb)
                    assert narrow_banded(one_wide) <= mb << 20  # (one block does fit at 16 bytes)
