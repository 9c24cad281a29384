"""Device groups, the pure-host part (no GPU): aesw_group_shard is sharding.shard_range, aesw_create_group refuses bad
arguments with the statuses include/aesw.h documents, and the group queries answer for something that is not a group."""
import ctypes as C

import numpy as np
import pytest

SIZES = [0, 1, 5, (1 << 16) + 5, (1 << 24) + 3]


def _shard(lib, g, n, i):
    first, count = C.c_uint64(), C.c_uint64()
    rc = lib.aesw_group_shard(g, n, i, C.byref(first), C.byref(count))
    return rc, int(first.value), int(count.value)


@pytest.mark.parametrize("g", range(1, 9))
def test_group_shard_equals_shard_range(pkg, g):
    lib = pkg.load_library()
    for n in SIZES:
        covered = 0
        for i in range(g):
            rc, first, count = _shard(lib, g, n, i)
            lo, hi = pkg.sharding.shard_range(n, i, g)
            assert rc == 0 and (first, first + count) == (lo, hi), (g, n, i)
            assert first == covered  # contiguous, in member order
            covered += count
            assert pkg.group_shard(g, n, i) == (lo, hi - lo)
        assert covered == n


def test_group_shard_large_n_does_not_overflow(pkg):
    lib = pkg.load_library()
    n = (1 << 63) + 12345
    for g in (3, 7, 8):
        assert sum(_shard(lib, g, n, i)[2] for i in range(g)) == n
        rc, first, count = _shard(lib, g, n, g - 1)
        assert rc == 0 and first == n * (g - 1) // g and first + count == n


def test_group_shard_refuses_bad_members(pkg):
    lib = pkg.load_library()
    INVALID = 1
    assert _shard(lib, 0, 10, 0)[0] == INVALID
    for g in (1, 3, 8):
        assert _shard(lib, g, 10, g)[0] == INVALID
        assert _shard(lib, g, 10, g + 5)[0] == INVALID
    first = C.c_uint64()
    assert lib.aesw_group_shard(2, 10, 0, C.byref(first), None) == INVALID
    with pytest.raises(pkg.AeswError):
        pkg.group_shard(0, 10, 0)


def _tables(pkg):
    return [np.ascontiguousarray(t, dtype=np.uint8) for t in pkg.reference_tables()]


def test_create_group_refuses_bad_arguments(pkg):
    lib = pkg.load_library()
    INVALID, NO_DEVICE = 1, 2
    tabs = _tables(pkg)
    tp = [t.ctypes.data_as(C.c_void_p) for t in tabs]
    devs = (C.c_int * 3)(0, 0, 0)
    h = C.c_void_p(1234)
    # count 0 with a device list
    assert lib.aesw_create_group(C.byref(h), devs, 0, *tp) == INVALID
    assert not h.value  # *out is cleared on failure
    # no place for the handle
    assert lib.aesw_create_group(None, devs, 2, *tp) == INVALID
    # a missing table
    assert lib.aesw_create_group(C.byref(h), devs, 2, tp[0], None, tp[2]) == INVALID
    # more members than a group holds
    many = (C.c_int * 65)(*([0] * 65))
    assert lib.aesw_create_group(C.byref(h), many, 65, *tp) == INVALID
    # a device out of range (or, without a GPU, no device at all)
    for bad in (-1, 1 << 20):
        d = (C.c_int * 2)(0, bad)
        h = C.c_void_p(1234)
        assert lib.aesw_create_group(C.byref(h), d, 2, *tp) == NO_DEVICE
        assert not h.value
    with pytest.raises(pkg.AeswError):
        pkg.Group([0, 1 << 20])


def test_group_queries_on_no_group(pkg):
    lib = pkg.load_library()
    assert lib.aesw_group_size(None) == 0
    assert not lib.aesw_group_member(None, 0)


def test_group_api_surface(pkg):
    """Group keeps Context's host-pointer methods and refuses the device-tensor ones without touching a device."""
    G = pkg.Group
    assert issubclass(G, pkg.Context)
    for name in ("encrypt_witness_host", "encrypt_witness_stream", "key_schedule_witness_host", "check_witness_host", "last_stream_stats",
                 "last_stream_check", "set_option", "get_option", "schedule_key_host", "lookup_table_host", "shard", "size"):
        assert hasattr(G, name), name
    g = G.__new__(G)  # no aesw_create_group: the refusal must not need one
    for name in ("encrypt_witness", "schedule_key", "key_schedule_witness", "check_witness", "alloc_witness", "alloc_columns", "expand_fr",
                 "assemble_advice", "encrypt_witness_batches", "lookup_table"):
        with pytest.raises(pkg.AeswError) as e:
            getattr(g, name)()
        assert e.value.args and "device pointers belong to one GPU" in str(e.value), name
