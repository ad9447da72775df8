"""The host side of the host-pointer block batch calls (lz4net_amd/csrc/lz4hip_hostbatch.hpp: the slice plan, the two staging images,
gather and scatter, the slice loop over kHostSlots sets of images, the shards of the multi-device form) on the CPU, over
tests/simt/emu_hostbatch.hpp's EmuStage: a stage without asynchrony whose copies out land only when the loop is told so, whose
pinned and device images are poisoned whenever their content is no longer owed to anybody, and which refuses a slot that is written
before its previous slice was drained.  The block codec is a stand-in that hands out arrays made here (or, once, the real wavefront
decoder under the SIMT emulator).  Every expected number below is a literal worked out by hand from the formulas the library had
before this code moved into the header (strides: max + 16 rounded up to 16; images: pieces rounded up to 256; slices: n / 2048
clamped to 1..6, the knob, the hint, then the byte limits), never taken from the code under test.  The `-m gpu` tests of
test_gpu_parity.py (test_host_batch_many_slices_and_layouts, test_multi_device_*) run the same code over the device."""
import ctypes as C

import numpy as np
import pytest

import emu_helpers as emu
from emu_helpers import addr, ref
from lz4net_amd._lib import E_ARGUMENT, E_DEVICE, Batch

GUARD = 64
UNTOUCHED = -12345678
COPY_IN, KERNELS, COPY_OUT, OUT_DONE, WAIT_OUT, QUIESCE = 2, 3, 4, 5, 6, 8          # EmuStage::Kind
PLAN = ["n", "max_src", "max_dst", "s_stride", "d_stride", "per_slice", "n_slices", "slots", "in_lens", "in_caps", "in_bytes", "out_res",
        "out_bytes", "last_first", "last_count", "rows_in", "tail_in", "rows_out", "tail_out"]


def clean(a):
    """bytes that are none of EmuStage's stale / poison / guard values, so that one of those in the caller's memory shows"""
    a = np.asarray(a, np.uint8).copy()
    a[np.isin(a, [0xDD, 0xEE, 0xBB, 0xC3])] = 0x11
    return a


def pattern(n):
    return clean((np.arange(n, dtype=np.int64) * 131 + 17) & 0xFF)


def limits(floor=-1, ceiling=-1, hinted=-1, pool_floor=-1, fail_at=-1, **kw):
    return emu.HostBatch(slice_floor=floor, slice_ceiling=ceiling, hinted_ceiling=hinted, pool_floor=pool_floor, fail_at=fail_at, **kw)


def plan(hb, knob=0, hint=0, lim=None):
    out = np.zeros(len(PLAN), np.int64)
    text = C.create_string_buffer(160)
    lim = lim or limits()
    rc = emu.hostbatch().emu_host_plan(ref(hb), knob, hint, ref(lim), addr(out), text)
    return rc, dict(zip(PLAN, (int(v) for v in out))), text.value.decode()


def uniform(n, src_len, dst_cap):
    """a batch of n rows of one length and capacity (the plan reads no row)"""
    return Batch(src=1, src_stride=src_len, src_len_all=src_len, dst=1, dst_stride=dst_cap, dst_cap_all=dst_cap, result=1, n_blocks=n)


# ---- the plan, with the library's limits ------------------------------------------------------------------------------------------------
def test_plan_knob_five_slices_of_64k_rows():
    """2 600 rows of 64 KiB in, compressBound out: strides 65 552 and 65 840 (131 392 a row), host_slices = 5 -> 520 a slice, inside
    the limits of 255 (32 MiB) and 4 086 (512 MiB) rows; the images: 520 x 65 552 = 34 087 040 -> 34 087 168, then 2 x 2 304."""
    rc, p, _ = plan(uniform(2600, 65536, 65809), knob=5)
    assert rc == 0
    assert (p["s_stride"], p["d_stride"], p["per_slice"], p["n_slices"], p["slots"]) == (65552, 65840, 520, 5, 4)
    assert (p["in_lens"], p["in_caps"], p["in_bytes"]) == (34087168, 34089472, 34091776)
    assert (p["out_res"], p["out_bytes"]) == (34236928, 34239232)
    assert (p["last_first"], p["last_count"]) == (2080, 520)
    assert (p["rows_in"], p["tail_in"], p["rows_out"], p["tail_out"]) == (34087040, 4608, 34236800, 2304)


def test_plan_default_six_slices():
    """16 384 rows, no knob: 16 384 / 2 048 = 8 -> 6 slices of ceil(16 384 / 6) = 2 731, the last one 16 384 - 5 x 2 731 = 2 729;
    a short slice copies its own rows and the whole tail."""
    rc, p, _ = plan(uniform(16384, 65809, 65536))
    assert rc == 0 and (p["s_stride"], p["d_stride"]) == (65840, 65552)
    assert (p["per_slice"], p["n_slices"], p["slots"], p["last_first"], p["last_count"]) == (2731, 6, 4, 13655, 2729)
    assert p["in_lens"] == 179809280 and p["in_bytes"] == 179809280 + 2 * 11008       # 2 731 x 65 840 = 179 809 040 -> + 240; 10 924 -> 11 008
    assert (p["rows_in"], p["tail_in"]) == (2729 * 65840, 22016)
    assert (p["rows_out"], p["tail_out"]) == (2729 * 65552, 11008)


@pytest.mark.parametrize("n, slices, per", [(2047, 1, 2047), (2048, 1, 2048), (4095, 1, 4095), (4096, 2, 2048), (12287, 5, 2458), (12288, 6, 2048)])
def test_plan_automatic_slice_counts(n, slices, per):
    rc, p, _ = plan(uniform(n, 65536, 65536))
    assert rc == 0 and (p["n_slices"], p["per_slice"]) == (slices, per)


def test_plan_hc_hint():
    """The LZ4HC hint of 16 384 blocks a slice holds while no row is longer than 64 KiB (below the 4 GiB ceiling: 32 688 rows of
    131 392 bytes), raises the 512 MiB ceiling with it, and is ignored for longer rows and next to the knob."""
    rc, p, _ = plan(uniform(16384, 65536, 65809), hint=16384)
    assert rc == 0 and (p["per_slice"], p["n_slices"], p["slots"]) == (16384, 1, 1)
    rc, p, _ = plan(uniform(40000, 65536, 65809), hint=40000)
    assert rc == 0 and (p["per_slice"], p["n_slices"]) == (32688, 2)
    rc, p, _ = plan(uniform(16384, 65537, 65809), hint=16384)
    assert rc == 0 and (p["s_stride"], p["per_slice"], p["n_slices"]) == (65568, 2731, 6)
    rc, p, _ = plan(uniform(16384, 65536, 65809), knob=8, hint=16384)
    assert rc == 0 and (p["per_slice"], p["n_slices"]) == (2048, 8)


def test_plan_small_rows_are_one_slice():
    """100 000 rows of 16 bytes: 64 bytes a row, the 32 MiB floor is 524 288 rows -> one slice"""
    rc, p, _ = plan(uniform(100000, 16, 16))
    assert rc == 0 and (p["s_stride"], p["d_stride"], p["per_slice"], p["n_slices"], p["slots"]) == (32, 32, 100000, 1, 1)
    assert (p["in_lens"], p["in_caps"], p["in_bytes"], p["out_res"], p["out_bytes"]) == (3200000, 3600128, 4000256, 3200000, 3600128)


def test_plan_ceiling_cuts_large_rows():
    """4 rows of 300 MiB in and out: one row is more than the 512 MiB ceiling allows (0 rows) -> slices of one row"""
    rc, p, _ = plan(uniform(4, 300 << 20, 300 << 20))
    assert rc == 0 and (p["per_slice"], p["n_slices"], p["slots"]) == (1, 4, 4)


def test_plan_empty_one_and_negative():
    rc, p, _ = plan(uniform(0, 5, 5))
    assert rc == 0 and p["n_slices"] == 0 and p["slots"] == 0
    rc, p, _ = plan(uniform(1, 5, 7))
    assert rc == 0 and (p["s_stride"], p["d_stride"], p["per_slice"], p["n_slices"], p["slots"]) == (32, 32, 1, 1, 1)
    assert (p["in_lens"], p["in_caps"], p["in_bytes"], p["out_res"], p["out_bytes"]) == (256, 512, 768, 256, 512)
    lens = np.array([3, 4, -1, 5], np.int32)
    hb = uniform(4, 0, 8)
    hb.src_len = addr(lens)
    rc, _, text = plan(hb)
    assert rc == E_ARGUMENT and text == "negative source length"
    # ... and the whole call refuses it before anything is staged
    res = np.full(4, UNTOUCHED, np.int32)
    hb.result = addr(res)
    r = limits()
    assert emu.hostbatch().emu_host_batch(ref(hb), ref(r)) == E_ARGUMENT
    assert r.error == b"negative source length" and r.reserves == 0 and r.log_n == 0 and (res == UNTOUCHED).all()
    hb.n_blocks = 0
    assert emu.hostbatch().emu_host_batch(ref(hb), ref(r)) == 0 and r.reserves == 0


def test_rules():
    L = emu.hostbatch()
    assert L.emu_host_rule(2, 0, 0, 0) == 4                                     # kHostSlots
    # fast encode: one residency round of ten blocks per CU = 2 560 on 256 CUs -> 7 equal slices of 16 384
    assert L.emu_host_rule(0, 16384, 0, 256) == 2341
    assert L.emu_host_rule(0, 4096, 0, 256) == 2048 and L.emu_host_rule(0, 4095, 0, 256) == 0 and L.emu_host_rule(0, 16384, 0, 0) == 0
    assert L.emu_host_rule(0, 100, 1, 256) == 16384 and L.emu_host_rule(0, 16384, 1, 0) == 16384       # LZ4HC: whatever the batch
    assert [L.emu_host_rule(1, n, hc, k) for n, hc, k in [(8191, 0, 0), (8192, 0, 0), (8192, 1, 0), (8192, 0, 1), (8192, 0, 3), (8192, 0, 20)]] == [1, 2, 1, 1, 3, 8]


# ---- the whole call -----------------------------------------------------------------------------------------------------------------------
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 2, 3, 5, 7, 11]                        # 20 ragged rows, longest 100
CAPS = [40, 0, 1, 16, 17, 33, 40, 5, 7, 39, 40, 12, 1, 0, 25, 31, 32, 2, 40, 9]                           # ... largest capacity 40
RESULTS = [40, 0, -3, 16, 99, 20, 0, -1, 7, 1, 45, 12, 1, 5, 24, 31, -77, 2, 39, 9]                       # over, under, at the capacity; failures


class Call:
    """A batch of ragged rows in guarded buffers, addressed by stride or by shuffled offsets, lengths and capacities per row or uniform,
    with the stand-in codec's arrays and the arrays the stage reports into."""

    def __init__(self, lens, caps, results, src_offsets, dst_offsets, uniform_len=None, uniform_cap=None, seed=1):
        n = self.n = len(lens)
        rng = np.random.default_rng(seed)
        self.lens = np.array([uniform_len] * n if uniform_len is not None else lens, np.int32)
        self.caps = np.array([uniform_cap] * n if uniform_cap is not None else caps, np.int32)
        self.results = np.array(results, np.int32)
        ss, ds = 112, 48                                                          # caller strides: not the staging's
        order_s, order_d = (rng.permutation(n), rng.permutation(n)) if n else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        self.src_at = np.array([(order_s[i] if src_offsets else i) * ss + (5 if src_offsets else 0) for i in range(n)], np.int64)
        self.dst_at = np.array([(order_d[i] if dst_offsets else i) * ds + (3 if dst_offsets else 0) for i in range(n)], np.int64)
        self.src = clean(rng.integers(0, 256, GUARD + n * ss + 16 + GUARD))
        self.dst = pattern(GUARD + n * ds + 16 + GUARD)
        self.stand = clean(rng.integers(0, 256, (max(n, 1), 48)))              # row r of the codec's output, capacity bytes of it
        self.res = np.full(max(n, 1), UNTOUCHED, np.int32)
        self.hb = Batch(src=addr(self.src, GUARD), src_stride=ss, dst=addr(self.dst, GUARD), dst_stride=ds, result=addr(self.res), n_blocks=n)
        if src_offsets:
            self.hb.src_off = addr(self.src_at)
        if dst_offsets:
            self.hb.dst_off = addr(self.dst_at)
        if uniform_len is None:
            self.hb.src_len = addr(self.lens)
        else:
            self.hb.src_len_all = uniform_len
        if uniform_cap is None:
            self.hb.dst_cap = addr(self.caps)
        else:
            self.hb.dst_cap_all = uniform_cap
        self.seen_src = np.zeros((max(n, 1), 128), np.uint8)
        self.seen_len = np.full(max(n, 1), UNTOUCHED, np.int32)
        self.seen_cap = np.full(max(n, 1), UNTOUCHED, np.int32)
        self.log = np.zeros((4096, 8), np.int64)

    def run_args(self, stand_results=None, stand_bytes=None, **kw):
        self.stand_results = self.results if stand_results is None else stand_results
        self.stand_bytes = self.stand if stand_bytes is None else stand_bytes
        kw.setdefault("floor", 0)
        kw.setdefault("ceiling", 1 << 20)
        kw.setdefault("hinted", 1 << 20)
        return limits(results=addr(self.stand_results), bytes=addr(self.stand_bytes), bytes_stride=self.stand_bytes.shape[1],
                      seen_src=addr(self.seen_src), seen_stride=128, seen_len=addr(self.seen_len), seen_cap=addr(self.seen_cap),
                      log=addr(self.log), log_cap=self.log.shape[0], **kw)

    def run(self, **kw):
        r = self.run_args(**kw)
        return emu.hostbatch().emu_host_batch(ref(self.hb), ref(r)), r

    def source_row(self, i):
        at = GUARD + int(self.src_at[i])
        return self.src[at:at + int(self.lens[i])]

    def expected_dst(self, by_result, rows=None):
        """the caller's output: the pattern, and for every row the bytes its rule owes it -- the result's (clamped to the capacity), or
        the whole capacity of a known-size decode that did not fail"""
        want = pattern(self.dst.size)
        for i in (range(self.n) if rows is None else rows):
            cap, res = int(self.caps[i]), int(self.results[i])
            nbytes = max(0, min(res, cap)) if by_result else (cap if res >= 0 else 0)
            at = GUARD + int(self.dst_at[i])
            want[at:at + nbytes] = self.stand[i, :nbytes]
        return want

    def records(self, r, kind):
        assert r.log_n <= self.log.shape[0]
        return [tuple(int(v) for v in rec[1:]) for rec in self.log[:r.log_n] if rec[0] == kind]


LAYOUTS = [dict(src_offsets=False, dst_offsets=False), dict(src_offsets=True, dst_offsets=False), dict(src_offsets=False, dst_offsets=True),
           dict(src_offsets=True, dst_offsets=True, uniform_len=48), dict(src_offsets=False, dst_offsets=True, uniform_cap=40),
           dict(src_offsets=True, dst_offsets=True, uniform_len=48, uniform_cap=40)]


@pytest.mark.parametrize("pool", [-1, 0], ids=["scatter-inline", "scatter-queued"])
@pytest.mark.parametrize("lag", [0, 1, 1000], ids=["landed-at-once", "landed-when-asked-twice", "never-landed-unasked"])
@pytest.mark.parametrize("knob, per_slice, n_slices", [(20, 1, 20), (10, 2, 10), (7, 3, 7)])
def test_whole_call(knob, per_slice, n_slices, lag, pool):
    """20 rows in 20, 10 and 7 slices (the last of 7 is short) over 4 slots, every layout and both result rules: results, every byte
    of the caller's output, what the kernels found staged, the device batch, the slots, EmuStage's guards and its refusals."""
    for layout in LAYOUTS:
        for by_result in (0, 1):
            c = Call(LENS, CAPS, RESULTS, **layout)
            rc, r = c.run(slices_knob=knob, lag=lag, pool_floor=pool, dst_len_is_result=by_result)
            what = (layout, by_result)
            assert rc == 0 and r.error == b"" and r.violations == 0 and r.intact == 1 and r.reserves == 1 and r.quiesces == 0, (what, r.error)
            assert np.array_equal(c.res, c.results), what
            assert np.array_equal(c.dst, c.expected_dst(by_result)), what
            assert np.array_equal(c.seen_len, c.lens) and np.array_equal(c.seen_cap, c.caps), what
            for i in range(c.n):
                assert np.array_equal(c.seen_src[i, :c.lens[i]], c.source_row(i)), (what, i)
            s_stride = 64 if "uniform_len" in layout else 128                   # 48 + 16 -> 64; 100 + 16 -> 128
            kernels = c.records(r, KERNELS)
            counts = [per_slice] * (20 // per_slice) + ([20 % per_slice] if 20 % per_slice else [])
            assert len(kernels) == n_slices == r.kernel_calls and r.rows_seen == 20
            for k, (slot, n_blocks, src_stride, dst_stride, src_len_all, dst_cap_all, flags) in enumerate(kernels):
                assert (slot, n_blocks, src_stride, dst_stride, dst_cap_all, flags) == (k % 4, counts[k], s_stride, 64, 0, 15), (what, k)
                assert src_len_all == (48 if "uniform_len" in layout else 100)
            # a slice is waited for exactly once, in order; with lag 1000 no out_done ever says yes
            assert [w[0] for w in c.records(r, WAIT_OUT)] == [k % 4 for k in range(n_slices)]
            if lag == 1000:
                assert not any(d[1] for d in c.records(r, OUT_DONE))


def test_copy_extents():
    """Ragged rows (strides 128 and 64) in slices of 3: images [384 -> 512 | 12 -> 256 | 256] = 1 024 and [192 -> 256 | 256] = 512; a
    slice copies its rows and the two tails, the last slice (2 rows) 256 and 128 bytes of rows."""
    c = Call(LENS, CAPS, RESULTS, False, False)
    rc, p, _ = plan(c.hb, knob=7, lim=limits(floor=0, ceiling=1 << 20, hinted=1 << 20))
    assert rc == 0 and (p["in_lens"], p["in_caps"], p["in_bytes"], p["out_res"], p["out_bytes"]) == (512, 768, 1024, 256, 512)
    assert (p["last_first"], p["last_count"], p["rows_in"], p["tail_in"], p["rows_out"], p["tail_out"]) == (18, 2, 256, 512, 128, 256)
    rc, r = c.run(slices_knob=7, lag=1)
    assert rc == 0
    ins, outs = c.records(r, COPY_IN), c.records(r, COPY_OUT)
    want_in, want_out = [], []
    for k in range(7):
        rows = 2 if k == 6 else 3
        want_in += [(k % 4, 0, 128 * rows), (k % 4, 512, 512)]
        want_out += [(k % 4, 0, 64 * rows), (k % 4, 256, 256)]
    assert [x[:3] for x in ins] == want_in and [x[:3] for x in outs] == want_out


def test_limits_set_the_slice():
    """The floor raises and the ceiling lowers what the knob asks for: rows of 128 + 64 = 192 bytes; a floor of 960 bytes is 5 rows, a
    ceiling of 400 bytes 2 rows; a hint of 7 rows under a hinted ceiling of 1 000 bytes is 5 rows."""
    c = Call(LENS, CAPS, RESULTS, False, False)
    for kw, knob, hint, per in [(dict(floor=960, ceiling=1 << 20), 20, 0, 5), (dict(floor=0, ceiling=400), 1, 0, 2), (dict(floor=0, ceiling=400, hinted=1000), 0, 7, 5),
                                (dict(floor=0, ceiling=2000, hinted=1000), 0, 7, 7)]:
        rc, p, _ = plan(c.hb, knob=knob, hint=hint, lim=limits(**kw))
        assert rc == 0 and p["per_slice"] == per, (kw, p)
        rc, r = c.run(slices_knob=knob, slice_hint=hint, lag=1, dst_len_is_result=1, **kw)
        assert rc == 0 and r.violations == 0 and r.kernel_calls == -(-20 // per) and np.array_equal(c.dst, c.expected_dst(1))


@pytest.mark.parametrize("pool", [-1, 0], ids=["scatter-inline", "scatter-queued"])
@pytest.mark.parametrize("lag, drained", [(1000, 0), (0, 1)])
def test_error_in_the_kernels_of_slice_two_of_six(lag, drained, pool):
    """12 rows in 6 slices; the kernels of slice 2 fail.  The call returns that code, waits for everything queued once, finishes the
    scatter of what it had drained (slice 0 where its copies had landed unasked) and leaves every other row as it was."""
    c = Call(LENS[:12], CAPS[:12], RESULTS[:12], True, True)
    rc, r = c.run(slices_knob=6, lag=lag, pool_floor=pool, fail_at=2, dst_len_is_result=1)
    assert rc == E_DEVICE and r.error == b"EmuStage: the kernels failed at row 4"
    assert r.quiesces == 1 and len(c.records(r, QUIESCE)) == 1 and r.kernel_calls == 3 and r.violations == 0 and r.intact == 1
    rows = list(range(2 * drained))
    assert np.array_equal(c.res[:len(rows)], c.results[:len(rows)]) and (c.res[len(rows):] == UNTOUCHED).all()
    assert np.array_equal(c.dst, c.expected_dst(1, rows))


@pytest.mark.parametrize("known", [1, 0])
def test_real_decoder(oracle, known):
    """12 blocks of the reference encoder through the library's loop in 3 slices, decoded by decode_kernel<known> under the emulator"""
    rng = np.random.default_rng(7)
    raws = [np.repeat(rng.integers(0, 256, 8 + 3 * i), 1 + i % 4).astype(np.uint8)[:20 + 11 * i] for i in range(12)]
    comps = [oracle.compress(x) for x in raws]
    lens = [len(x) for x in comps]
    caps = [len(x) + (0 if known else 9) for x in raws]
    c = Call(lens, caps, [0] * 12, True, False)
    ss = 400
    c.src = clean(np.zeros(GUARD + 12 * ss + GUARD))
    c.src_at = np.arange(12, dtype=np.int64) * ss
    for i, x in enumerate(comps):
        c.src[GUARD + i * ss:GUARD + i * ss + len(x)] = x
    c.dst = pattern(GUARD + 12 * 256 + GUARD)
    c.hb.src, c.hb.src_off, c.hb.dst, c.hb.dst_stride = addr(c.src, GUARD), addr(c.src_at), addr(c.dst, GUARD), 256
    c.seen_src = np.zeros((12, 512), np.uint8)
    r = c.run_args(slices_knob=3, lag=1, decoder=1 if known else 2, dst_len_is_result=0 if known else 1)
    r.seen_stride = 512
    r.seen_src = addr(c.seen_src)
    assert emu.hostbatch().emu_host_batch(ref(c.hb), ref(r)) == 0 and r.violations == 0 and r.intact == 1 and r.kernel_calls == 3
    assert list(c.res) == (lens if known else [len(x) for x in raws])
    want = pattern(c.dst.size)
    for i, x in enumerate(raws):
        want[GUARD + i * 256:GUARD + i * 256 + len(x)] = x
    assert np.array_equal(c.dst, want)


# ---- the shards ---------------------------------------------------------------------------------------------------------------------------
def shard_call(c, nd, fail_shards=0, **kw):
    """the stand-in's rows in the order the shards run: shard 0's rows, shard 1's, ..."""
    order = [i for k in range(nd) for i in range(k, c.n, nd)]
    stand_results = np.array([c.results[i] for i in order] + [0], np.int32)
    stand_bytes = np.ascontiguousarray(c.stand[order + [0]])
    r = c.run_args(stand_results, stand_bytes, lag=1, **kw)
    devs = np.arange(10, 10 + nd, dtype=np.int32)
    rows, reserves = np.full(nd, -1, np.int64), np.full(nd, -1, np.int64)
    rc = emu.hostbatch().emu_host_shards(ref(c.hb), nd, addr(devs), fail_shards, ref(r), addr(rows), addr(reserves))
    return rc, r, rows, reserves


@pytest.mark.parametrize("nd", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 5, 17])
def test_shards(n, nd):
    """Block i belongs to shard i mod nd: shard k has the blocks k, k + nd, ... (none when n <= k: nothing is staged for it), and
    result j of shard k lands at j * nd + k."""
    for layout in (LAYOUTS[0], LAYOUTS[3]):
        for by_result in (0, 1):
            c = Call(LENS[:n], CAPS[:n], RESULTS[:n], **layout)
            rc, r, rows, reserves = shard_call(c, nd, slices_knob=3, dst_len_is_result=by_result)
            assert rc == 0 and r.error == b"" and r.violations == 0 and r.intact == 1
            assert list(rows) == [len(range(k, n, nd)) for k in range(nd)] and list(reserves) == [int(k < n) for k in range(nd)]
            assert np.array_equal(c.res[:n], c.results[:n])
            assert np.array_equal(c.dst, c.expected_dst(by_result))


def test_failing_shards_report_the_first():
    """5 blocks on 3 devices (10, 11, 12); shards 1 and 2 fail: the call reports shard 1's failure under its device's name; shard
    0's results (blocks 0 and 3) have landed, no other."""
    c = Call(LENS[:5], CAPS[:5], RESULTS[:5], False, False)
    rc, r, rows, _ = shard_call(c, 3, fail_shards=0b110, dst_len_is_result=1)
    assert rc == E_DEVICE and r.error == b"device 11: EmuStage: the kernels failed at row 2" and list(rows) == [2, 2, 1]
    assert [int(v) for v in c.res[:5]] == [RESULTS[0], UNTOUCHED, UNTOUCHED, RESULTS[3], UNTOUCHED]
