"""Device tier of the SST decompression / checksum tests: files written by
codec_cases.write_sst from full-format Snappy and LZ4 streams go through
yb_gpu_scan_feed_sst (k_crc32c, then k_snappy) and must give, bit for bit,
what the same scan gives over the raw blocks fed directly, and what the CPU
oracle gives: COUNT(*), SUM, MIN and MAX of every integer column and every
row with its keys and values. One wrong decompressed byte in any entry
changes a key or a value.

The malformed streams reach the device only in files whose checksums are
correct, and only streams that the stand-alone sanitizer driver
(csrc/codec_sim_main.cc) has run clean on the CPU: they are inputs the
decoders are designed to reject, each confined to its slot by the decoder's
own bounds checks.

Not covered: the grid-stride loop of k_snappy and k_crc32c runs a second
iteration only above 4096 * 256 = 1,048,576 blocks, which no test-sized file
reaches. Of the files whose data bytes are corrupted and whose CRC is then
recomputed, the device is fed only those whose flipped bit leaves the block
well formed (codec_cases.harmless_flip: a bit of a value); the flips at the
first and the last bytes of a block are verified with a recomputed CRC on
the host tier only (test_codec_streams.py), since on the device they would
hand a structurally broken block (preamble, restart count) to the scan
set-up, which is not what these tests are about.

A type-0 block is copied into its slot, so a byte the copy misses shows
whatever the buffer held before. Every feed of a file of the noise tablet
therefore follows feeds of the same blocks in reverse order (feed_file's
poison), which leave other bytes in the buffers the allocator may hand out
again.
"""
import functools

import pytest

import codec_cases as cc
import ybgpu as y

pytestmark = pytest.mark.gpu

KEYS = [(t, c, m) for t in cc.TABLETS for c in (cc.SNAPPY, cc.LZ4)
        for m in cc.MODES]
IDS = ["%s-%s-%s" % (t, cc.CODEC_NAMES[c], m) for t, c, m in KEYS]


def _agg_sets(schema):
    """COUNT(*), SUM, MIN, MAX of every integer column, in sets of at most
    MAX_AGGS; COUNT of the other columns."""
    ints = [c for c in range(schema.num_value_cols)
            if schema.value_cols[c].dtype == y.T_INT64]
    rest = [c for c in range(schema.num_value_cols) if c not in ints]
    first = [(y.AGG_COUNT_STAR, 0)] + [(y.AGG_SUM_INT64, c) for c in ints] + \
        [(y.AGG_COUNT, c) for c in rest]
    sets = [first, [(y.AGG_MIN_INT64, c) for c in ints],
            [(y.AGG_MAX_INT64, c) for c in ints]]
    assert all(len(s) <= y.MAX_AGGS for s in sets)
    return sets


def _spec(schema, aggs=(), emit=False):
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(cc.READ_MICROS)
    spec.num_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        spec.aggs[i] = y.Agg(op, col)
    spec.emit_rows = 1 if emit else 0
    return spec


def _flat(res, n_aggs):
    return (res.rows_scanned, res.rows_matched,
            tuple((bool(res.aggs[i].is_null),
                   None if res.aggs[i].is_null else res.aggs[i].value_i64)
                  for i in range(n_aggs)))


def gpu_results(schema, feed):
    """(aggregate tuples per set, every row) of a scan that feed() fills."""
    from gpu_scan import GpuScan
    aggs_out = []
    for aggs in _agg_sets(schema):
        s = GpuScan(_spec(schema, aggs))
        try:
            feed(s)
            s.execute()
            aggs_out.append(_flat(s.aggregates(), len(aggs)))
        finally:
            s.close()
    s = GpuScan(_spec(schema, emit=True))
    try:
        feed(s)
        rows = s.batch_rows()
    finally:
        s.close()
    return aggs_out, rows


def feed_file(sst, verify=True, poison=None):
    """poison: a file of the same decompressed size whose blocks lie
    elsewhere. It is fed to a few scans that are open at the same time and
    then closed, right before every feed of sst, so that a device buffer the
    allocator hands out again holds other bytes than the right ones: a slot
    byte the kernel fails to write cannot come out correct by accident."""
    ptr, size = cc.sst_buffer(sst)
    if poison is None:
        return lambda s: s.feed_sst(ptr, size, verify=verify)
    pptr, psize = cc.sst_buffer(poison)

    def feed(s):
        from gpu_scan import GpuScan
        others = [GpuScan(s._spec) for _ in range(3)]
        try:
            for o in others:
                o.feed_sst(pptr, psize, verify=True)
        finally:
            for o in others:
                o.close()
        s.feed_sst(ptr, size, verify=verify)
    return feed


def poison_file(entries):
    """The same blocks in reverse order: every block is well formed, the
    decompressed size is the same, and (the block sizes differ) every slot
    begins and ends somewhere else."""
    sizes = [len(raw) for _, _, raw in entries]
    assert len(set(sizes)) > 8
    sst, _ = cc.write_sst([(s, bt) for s, bt, _ in reversed(entries)])
    return sst


@functools.lru_cache(maxsize=None)
def reference(tablet):
    """Computed once per tablet: the raw blocks fed directly, and the CPU
    oracle over the raw blocks."""
    t = cc.tablets()[tablet]
    raw = gpu_results(t["schema"], lambda s: s.feed_blocks_host(
        t["data"], t["offsets"], t["n_blocks"], t["total"]))
    osc = y.orcl_schema_from(t["schema"])
    oaggs = []
    for aggs in _agg_sets(t["schema"]):
        ospec = y.OrclScanSpec()
        ospec.read_time = y.orcl_read_time(cc.READ_MICROS)
        ospec.num_aggs = len(aggs)
        for i, (op, col) in enumerate(aggs):
            ospec.aggs[i] = y.OrclAgg(op, col)
        ores, _ = y.orcl_scan(t["data"], t["offsets"], t["n_blocks"], osc,
                              ospec)
        oaggs.append(_flat(ores, len(aggs)))
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(cc.READ_MICROS)
    _, orows = y.orcl_scan(t["data"], t["offsets"], t["n_blocks"], osc, ospec,
                           collect_rows=True)
    return {"raw": raw, "oracle": (oaggs, orows)}


def check_parity(tablet, entries, verify=True):
    t = cc.tablets()[tablet]
    sst, _ = cc.write_sst([(s, bt) for s, bt, _ in entries])
    # type-0 blocks are copied, not decoded: what a missed byte would show
    # is whatever the buffer held before
    poison = poison_file(entries) if tablet == "noise" else None
    got_aggs, got_rows = gpu_results(t["schema"],
                                     feed_file(sst, verify, poison))
    ref = reference(tablet)
    assert len(got_rows) == len(ref["oracle"][1]) > 0
    assert got_aggs == ref["raw"][0]
    assert got_aggs == ref["oracle"][0]
    assert got_rows == ref["raw"][1]
    assert got_rows == ref["oracle"][1]


@pytest.mark.parametrize("tablet", cc.TABLETS)
def test_raw_fed_scan_equals_oracle(tablet):
    ref = reference(tablet)
    assert ref["raw"][0] == ref["oracle"][0]
    assert ref["raw"][1] == ref["oracle"][1]
    assert ref["raw"][0][0][0] == len(ref["raw"][1]) > 0


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_feed_sst_parity(key):
    check_parity(key[0], cc.corpus_entry(*key))


def test_feed_sst_parity_unverified():
    check_parity("small", cc.corpus_entry("small", cc.SNAPPY, "mix"),
                 verify=False)


def test_slot_isolation_alternating_types():
    """Types 0 / 1 / 4 alternate in one file: every branch of k_snappy
    writes a slot that begins at an arbitrary byte offset, and the full row
    fetch shows that none of them touched a neighbour's bytes."""
    entries = cc.alternating_entry()
    assert {bt for _, bt, _ in entries} == {0, cc.SNAPPY, cc.LZ4}
    dst, aligns = 0, set()
    for _, bt, raw in entries:
        aligns.add((bt, dst % 8))
        dst += len(raw)
    for bt in (0, cc.SNAPPY, cc.LZ4):
        assert len({a for b, a in aligns if b == bt}) >= 4
    check_parity("noise", entries)


def _small_snappy():
    entries = cc.corpus_entry("small", cc.SNAPPY, "real")
    return cc.write_sst([(s, bt) for s, bt, _ in entries])


def _open(schema):
    from gpu_scan import GpuScan
    return GpuScan(_spec(schema, [(y.AGG_COUNT_STAR, 0)]))


def test_device_crc_catches_every_flip():
    schema = cc.tablets()["small"]["schema"]
    sst, handles = _small_snappy()
    picked, flips = cc.crc_flips(sst, handles)
    assert {(handles[i][1] + 1) % 4 for i in picked} == {0, 1, 2, 3}
    assert len({handles[i][0] % 8 for i in picked}) >= 4
    assert len(flips) == 36
    # the file as written verifies on the device
    s = _open(schema)
    try:
        feed_file(sst)(s)
    finally:
        s.close()
    for name, pos, mask in flips:
        bad = bytearray(sst)
        bad[pos] ^= mask
        s = _open(schema)
        try:
            with pytest.raises(RuntimeError, match="checksum"):
                feed_file(bytes(bad))(s)
        finally:
            s.close()
    # a flipped bit that leaves the block well formed: the file fails the
    # checksum as it is, and with the CRC recomputed it feeds, and every row
    # is what the oracle reads from the changed blocks
    entries = cc.corpus_entry("small", cc.SNAPPY, "real")
    for i in picked:
        pos, blocks = cc.harmless_flip(schema, entries, i)
        bad = bytearray(sst)
        bad[handles[i][0] + pos] ^= 0x01
        s = _open(schema)
        try:
            with pytest.raises(RuntimeError, match="checksum"):
                feed_file(bytes(bad))(s)
        finally:
            s.close()
        cc.refresh_trailer(bad, handles[i])
        _, rows = gpu_results(schema, feed_file(bytes(bad)))
        assert rows == cc.oracle_rows(schema, blocks)
        assert rows != reference("small")["oracle"][1]


HOST_CAUGHT = {"empty", "truncated_preamble", "truncated_preamble_2",
               "preamble_6_bytes", "preamble_above_32_bits"}


def test_malformed_streams_rejected_on_device():
    """A good block, then the malformed stream with a CORRECT checksum and
    a consistent handle. The Snappy slot is what the stream's own preamble
    states; the LZ4 slot is the framed length."""
    schema = cc.tablets()["small"]["schema"]
    good = cc.corpus_entry("small", cc.SNAPPY, "real")[0]
    fed = 0
    for name, codec, stream, cap in cc.malformed():
        ulen = cap
        if codec == cc.SNAPPY and name not in HOST_CAUGHT:
            ulen = cc.snappy_ulen(stream)
        if ulen > 1 << 20:
            continue    # the feed path sizes its allocation from it
        sst, _ = cc.write_sst([(good[0], good[1]), (stream, codec)])
        want = ("corrupt compressed-block length preamble"
                if name in HOST_CAUGHT else "block decompression failed")
        s = _open(schema)
        try:
            with pytest.raises(RuntimeError, match=want):
                feed_file(sst)(s)
        finally:
            s.close()
        fed += 1
    assert fed == len(cc.malformed())   # nothing above 1 MiB today
    # the device and the process are as before: a fresh scan still works
    check_parity("small", cc.corpus_entry("small", cc.SNAPPY, "real"))
