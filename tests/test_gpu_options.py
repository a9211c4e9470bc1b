"""The option surface of a context (curvis_ctx_set_option / curvis_ctx_get_option), key by key.

The key lists below are written out from the two else-if chains the library had before its option table: 22 keys that
are set and read back, two test hooks that can be set but not read, 19 statistics that can be read but not set.  A key
that is not writable is refused exactly like a key that does not exist ("unknown option <key>"); a key that is not
readable is refused without touching the error text.  The hooks are only ever given 0 here: what they do when armed is
tests/test_gpu_parity.py's business."""
import ctypes as C

import pytest

import curvis_amd
from curvis_amd import _abi

pytestmark = pytest.mark.gpu

# key -> (default of a fresh context, a legal value that is not the default)
READ_WRITE = {
    "variant": (-1, 1),
    "refill_threshold": (16, 32),
    "blocks_per_cu": (0, 2),
    "block_threads": (0, 128),
    "relay_segment": (0, 512),
    "relay_max_hops": (0, 3),
    "relay_max_parks": (0, 5),
    "relay_recheck_every": (1024, 7),
    "async_download": (0, 1),
    "async_streams": (0, 1),
    "relay_max_frames": (8, 4),
    "relay_min_blocks": (-1, 100),
    "relay_verify": (0, 1),
    "relay_auto_verify": (1, 0),
    "relay_disabled": (0, 1),
    "fast_math": (1, 0),
    "fuse_shade": (1, 0),
    "device_sampler": (-1, 1),
    "device_sampler_min_frames": (48, 16),
    "sampling_speculation": (-1, 3),
    "sampling_speculation_first": (-1, 2),
    "max_store_bytes": (8 << 30, 1 << 20),
}
WRITE_ONLY = ("relay_test_corrupt", "relay_test_fault")
READ_ONLY = (
    "relay_mismatches", "relay_verified_shapes", "relay_checks", "last_png_stream_bytes", "streams_pending",
    "downloads_overlapped", "download_pending", "relay_fallbacks", "last_frames", "last_relay_launches",
    "last_relay_parks", "last_relay_waiters", "last_sampler_path", "last_sampling_chains", "last_sampling_prefetched",
    "prefetches", "prefetch_hits", "last_sampling_launches", "last_sampling_evaluated",
)


@pytest.fixture()
def ctx():
    c = curvis_amd.Context(0)
    yield c
    c.close()


def raw_set(c, key, value):
    return _abi.lib().curvis_ctx_set_option(c._h, key.encode(), int(value))


def raw_get(c, key):
    v = C.c_int64(-12345)
    return _abi.lib().curvis_ctx_get_option(c._h, key.encode(), C.byref(v)), v.value


def last_error(c):
    return (_abi.lib().curvis_last_error(c._h) or b"").decode()


def test_key_lists_are_what_the_issue_counts():
    assert len(READ_WRITE) == 22 and len(WRITE_ONLY) == 2 and len(READ_ONLY) == 19
    assert len(set(READ_WRITE) | set(WRITE_ONLY) | set(READ_ONLY)) == 43


@pytest.mark.parametrize("key", sorted(READ_WRITE))
def test_read_write_key_round_trips(ctx, key):
    default, other = READ_WRITE[key]
    assert raw_get(ctx, key) == (0, default)
    assert raw_set(ctx, key, other) == 0
    assert raw_get(ctx, key) == (0, other)
    others = {k: raw_get(ctx, k)[1] for k in READ_WRITE if k != key}
    assert others == {k: READ_WRITE[k][0] for k in others}, "setting %s changed another option" % key
    assert raw_set(ctx, key, default) == 0
    assert raw_get(ctx, key) == (0, default)


@pytest.mark.parametrize("key", WRITE_ONLY)
def test_test_hooks_are_write_only(ctx, key):
    assert raw_set(ctx, key, 0) == 0
    before = last_error(ctx)
    assert raw_get(ctx, key) == (_abi.E_INVALID, -12345)
    assert last_error(ctx) == before


@pytest.mark.parametrize("key", READ_ONLY)
def test_statistics_are_read_only(ctx, key):
    rc, v = raw_get(ctx, key)
    assert rc == 0 and v == 0  # a fresh context has rendered, checked, prefetched and downloaded nothing
    assert raw_set(ctx, key, 1) == _abi.E_INVALID
    assert last_error(ctx) == "unknown option " + key
    assert raw_get(ctx, key) == (0, 0)


def test_invented_key_fails_both_ways(ctx):
    key = "no_such_option"
    assert raw_set(ctx, "variant", 1) == 0
    before = last_error(ctx)
    assert raw_get(ctx, key) == (_abi.E_INVALID, -12345)
    assert last_error(ctx) == before, "get_option of an unknown key leaves the error text alone"
    assert raw_set(ctx, key, 1) == _abi.E_INVALID
    assert last_error(ctx) == "unknown option " + key
    with pytest.raises(curvis_amd.CurvisError, match="unknown option " + key):
        ctx.set_option(key, 1)


def test_values_the_setters_normalise(ctx):
    ctx.set_option("device_sampler_min_frames", 0)
    assert ctx.get_option("device_sampler_min_frames") == 1
    ctx.set_option("device_sampler_min_frames", -5)
    assert ctx.get_option("device_sampler_min_frames") == 1
    for key in ("async_download", "async_streams"):
        ctx.set_option(key, 7)
        assert ctx.get_option(key) == 1
        ctx.set_option(key, 0)  # waits for what is in flight (nothing), then clears the flag
        assert ctx.get_option(key) == 0
    # everything but relay_min_blocks and max_store_bytes goes through an int
    ctx.set_option("relay_min_blocks", 1 << 40)
    assert ctx.get_option("relay_min_blocks") == 1 << 40
    ctx.set_option("max_store_bytes", 1 << 40)
    assert ctx.get_option("max_store_bytes") == 1 << 40
    ctx.set_option("relay_segment", (1 << 32) + 9)
    assert ctx.get_option("relay_segment") == 9
