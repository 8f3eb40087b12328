"""Where the node pipeline's trace kernel leaves what finalize reads (csrc/launch.h skr_trace_header_row / _bit, csrc/render_nodes.hip
plan_for), asked of the library's own arithmetic through skr_trace_header_map (internal; no device involved).  For a level of `nodes`
nodes with N children each (PP = ceil(N / 2) sibling pairs): every (node, pair) has a (header row, ballot bit) of its own, every row
lies inside the table the plan allocates, and the 64 record regions — region r receives the rows = r (mod 64), each row's wave at most
128 hits (64 lanes x 2 children) — hold the worst case."""
import ctypes as C

import numpy as np
import pytest

import skele_raytracer_amd as skr

NODES = (0, 1, 63, 64, 65, 4097)
CHILDREN = (1, 2, 3, 16, 255, 256)


def header_map(nodes, n):
    fn = skr.lib().skr_trace_header_map
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    pp = (n + 1) // 2
    out = (C.c_uint64 * 3)()
    rows = np.full(max(nodes * pp, 1), 0xFFFFFFFF, np.uint32)
    bits = np.full(max(nodes * pp, 1), 0xFFFFFFFF, np.uint32)
    got = fn(nodes, n, out, rows.ctypes.data_as(C.POINTER(C.c_uint32)), bits.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert got == pp
    return pp, int(out[0]), int(out[1]), int(out[2]), rows[:nodes * pp].astype(np.uint64), bits[:nodes * pp].astype(np.uint64)


@pytest.mark.parametrize("n", CHILDREN)
@pytest.mark.parametrize("nodes", NODES)
def test_rows_bits_and_capacity(nodes, n):
    pp, used, alloc, cap, rows, bits = header_map(nodes, n)
    assert used <= alloc
    if nodes == 0:
        assert used == 0
        return
    assert rows.size == nodes * pp
    assert int(bits.max()) < 64
    slots = rows * np.uint64(64) + bits
    assert np.unique(slots).size == slots.size, "two sibling pairs share a header row and bit"
    assert int(rows.max()) < used <= alloc, (int(rows.max()), used, alloc)
    # 128 hits per row at most, to region row & 63
    per_region = np.bincount((np.arange(used) & 63), minlength=64)
    assert cap >= 128 * int(per_region.max()), (cap, per_region.max())
    assert cap * 64 >= 128 * used
    # the mapping the kernels are built with: a wave is 64 consecutive nodes (one row per pair), or 64 consecutive pairs
    by_node = np.array_equal(rows.reshape(nodes, pp)[:, 0], (np.arange(nodes, dtype=np.uint64) >> np.uint64(6)) * np.uint64(pp))
    if by_node:
        assert np.array_equal(bits.reshape(nodes, pp), np.broadcast_to((np.arange(nodes, dtype=np.uint64) & np.uint64(63))[:, None], (nodes, pp)))
        assert np.array_equal(rows.reshape(nodes, pp), rows.reshape(nodes, pp)[:, :1] + np.arange(pp, dtype=np.uint64)[None, :])
        assert used == (nodes + 63) // 64 * pp
