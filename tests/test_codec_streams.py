"""Host tier of the SST decompression / checksum tests: the decoders of
snappy_dev.h and lz4_dev.h (the functions the GPU kernel compiles) against
the independent restatement, encoders and SST writer of codec_cases.py, on
full-format streams. Every comparison is byte-exact; the census and the
residue conditions are asserted, so the corpus cannot quietly lose the
elements it exists for."""
import ctypes as C

import pytest

import codec_cases as cc
import ybgpu as y

KEYS = [(t, c, m) for t in cc.TABLETS for c in (cc.SNAPPY, cc.LZ4)
        for m in cc.MODES]
IDS = ["%s-%s-%s" % (t, cc.CODEC_NAMES[c], m) for t, c, m in KEYS]


def host_decode(stored, btype, cap, guard=True):
    """What the kernel does with one stored block, on the host."""
    if btype == cc.SNAPPY:
        return y.snappy_uncompress(stored, cap, guard=guard)
    if btype == cc.LZ4:
        _, o = cc.read_uvarint32(stored)
        return y.lz4_uncompress(stored[o:], cap, guard=guard)
    return stored


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_decode_exact(key):
    """cap == len(raw) exactly: no slack for an overrun to hide in, and the
    guard bytes behind the destination must survive."""
    entries = cc.corpus_entry(*key)
    assert any(btype == key[1] for _, btype, _ in entries)
    for i, (stored, btype, raw) in enumerate(entries):
        assert host_decode(stored, btype, len(raw)) == raw, (key, i)


def test_alternating_decode_exact():
    entries = cc.alternating_entry()
    assert {t for _, t, _ in entries} == {0, cc.SNAPPY, cc.LZ4}
    for i, (stored, btype, raw) in enumerate(entries):
        assert host_decode(stored, btype, len(raw)) == raw, i


def test_tablet_shapes():
    """The properties the tablets are built for."""
    t = cc.tablets()
    assert t["small"]["n_blocks"] > 256          # a second workgroup
    small = cc.corpus_entry("small", cc.SNAPPY, "real")
    assert all(len(cc.uvarint(len(raw))) == 2 for _, _, raw in small)
    assert all(btype == cc.SNAPPY for _, btype, _ in small)
    big = t["big"]["blocks"]
    assert any(len(b) > 65536 for b in big) and len(big) >= 2
    assert all(len(cc.uvarint(len(b))) == 3 for b in big)
    # noise: type-0 blocks between compressed neighbours, with destination
    # slots off the 8-byte grid and every length tail of the u64 copy
    for codec in (cc.SNAPPY, cc.LZ4):
        entries = cc.corpus_entry("noise", codec, "real")
        types = [btype for _, btype, _ in entries]
        assert any(types[i] == 0 and types[i - 1] and types[i + 1]
                   for i in range(1, len(types) - 1))
        dst, aligns, tails = 0, set(), set()
        for stored, btype, raw in entries:
            if btype == 0:
                aligns.add(dst % 8)
                tails.add(len(raw) % 8)
            dst += len(raw)
        assert len(aligns) >= 4 and tails == set(range(8)), (aligns, tails)
    kept_raw = {}
    for key in KEYS:
        if key[0] == "noise":
            types = [btype for _, btype, _ in cc.corpus_entry(*key)]
            kept_raw[key] = sum(t == 0 and i % 3 != 2
                                for i, t in enumerate(types))
            print("noise", key, "blocks", len(types), "stored raw because "
                  "they did not shrink", kept_raw[key])
    # besides the forced every-third block, some blocks did not shrink: for
    # each codec at least one file has them, next to compressed ones
    for codec in (cc.SNAPPY, cc.LZ4):
        assert any(0 < n < 2 * len(types) // 3
                   for k, n in kept_raw.items() if k[1] == codec), kept_raw


def test_census_snappy():
    total = dict.fromkeys(cc.SNAPPY_KEYS, 0)
    for t in cc.TABLETS:
        for m in cc.MODES:
            got = cc.census_sum(cc.corpus_entry(t, cc.SNAPPY, m), cc.SNAPPY)
            print("census snappy", t, m, got)
            for k, v in got.items():
                total[k] += v
            if m == "real":
                copies = got["copy1"] + got["copy2"] + got["copy4"]
                # the property of real Snappy that motivates these tests
                assert copies and 2 * got["copy1"] >= copies, (t, got)
    for k in cc.SNAPPY_KEYS:
        assert total[k] > 0, (k, total)


def test_census_lz4():
    total = dict.fromkeys(cc.LZ4_KEYS, 0)
    for t in cc.TABLETS:
        for m in cc.MODES:
            got = cc.census_sum(cc.corpus_entry(t, cc.LZ4, m), cc.LZ4)
            print("census lz4", t, m, got)
            for k, v in got.items():
                total[k] += v
    for k in cc.LZ4_KEYS:
        assert total[k] > 0, (k, total)


def test_project_compressors_conform():
    """The project's own compressors against the independent decoders."""
    for name, t in cc.tablets().items():
        blocks = t["blocks"]
        for raw in blocks[:40] + blocks[-2:]:
            assert cc.ref_snappy_decode(y.snappy_compress(raw)) == raw, name
            framed = cc.uvarint(len(raw)) + y.lz4_compress(raw)
            assert cc.ref_lz4_decode(framed) == raw, name


MALFORMED = cc.malformed()


def test_malformed_list_covers_the_bounds_checks():
    names = [m[0] for m in MALFORMED]
    assert len(set(names)) == len(names)
    assert sum(m[1] == cc.SNAPPY for m in MALFORMED) >= 17
    assert sum(m[1] == cc.LZ4 for m in MALFORMED) >= 9


@pytest.mark.parametrize("case", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_rejected(case):
    _name, codec, stream, cap = case
    # the reference rejects it: the case IS malformed
    with pytest.raises(cc.CodecError):
        (cc.ref_snappy_decode if codec == cc.SNAPPY
         else cc.ref_lz4_decode)(stream)
    # the host decoder rejects it and stays inside its cap bytes
    if codec == cc.SNAPPY:
        with pytest.raises(RuntimeError, match="snappy_uncompress failed"):
            y.snappy_uncompress(stream, cap, guard=True)
        return
    framed, o = cc.read_uvarint32(stream)
    assert framed == cap
    try:
        out = y.lz4_uncompress(stream[o:], cap, guard=True)
    except RuntimeError as e:
        assert "lz4_uncompress failed" in str(e)
    else:
        assert len(out) != cap   # the kernel's test: returned != framed


def _small_file():
    entries = cc.corpus_entry("small", cc.SNAPPY, "real")
    return cc.write_sst([(s, t) for s, t, _ in entries])


@pytest.mark.parametrize("key", KEYS + ["alternating"],
                         ids=IDS + ["alternating"])
def test_written_files_parse(key):
    entries = (cc.alternating_entry() if key == "alternating"
               else cc.corpus_entry(*key))
    sst, handles = cc.write_sst([(s, t) for s, t, _ in entries])
    offs, szs = y.sst_index(sst, verify=True)
    assert list(zip(offs, szs)) == handles
    assert [sst[o + s] for o, s in handles] == [t for _, t, _ in entries]


def test_trailer_flips_fail_checksum():
    sst, handles = _small_file()
    picked, flips = cc.crc_flips(sst, handles)
    assert {(handles[i][1] + 1) % 4 for i in picked} == {0, 1, 2, 3}
    assert len(flips) == 9 * 4
    for name, pos, mask in flips:
        bad = bytearray(sst)
        bad[pos] ^= mask
        with pytest.raises(RuntimeError, match="checksum"):
            y.sst_index(bytes(bad), verify=True)
        # unverified, the same file still parses to the same handles
        offs, szs = y.sst_index(bytes(bad), verify=False)
        assert list(zip(offs, szs)) == handles, name
    # the flipped data bytes with the CRC recomputed verify again
    for i in picked:
        off, size = handles[i]
        for pos in (off, off + size - 1, off + size - 2, off + size - 3):
            fixed = bytearray(sst)
            fixed[pos] ^= 0x01
            cc.refresh_trailer(fixed, handles[i])
            y.sst_index(bytes(fixed), verify=True)


def test_harmless_flips_exist_and_decode():
    """The flips the device tier feeds with a recomputed CRC: one per
    attacked block, after which the host decoder gives the changed block."""
    entries = cc.corpus_entry("small", cc.SNAPPY, "real")
    sst, handles = _small_file()
    picked, _ = cc.crc_flips(sst, handles)
    schema = cc.tablets()["small"]["schema"]
    for i in picked:
        pos, blocks = cc.harmless_flip(schema, entries, i)
        bad = bytearray(entries[i][0])
        bad[pos] ^= 0x01
        assert blocks[i] != entries[i][2]
        assert host_decode(bytes(bad), cc.SNAPPY, len(blocks[i])) == blocks[i]


@pytest.mark.parametrize("tablet", cc.TABLETS)
def test_emitted_rows_in_key_order(tablet):
    """Every row of the tablet, in tablet key order, from the simulator's
    emit path: the reference of the device tier's row comparison. The big
    tablet's blocks exceed 64 KB, so an entry's offset inside its block
    does not fit 16 bits of the row's sort key."""
    t = cc.tablets()[tablet]
    spec = y.ScanSpec()
    spec.schema = t["schema"]
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(cc.READ_MICROS)
    spec.emit_rows = 1
    got = y.sim_emit(spec, t["data"], t["offsets"], t["n_blocks"])
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(cc.READ_MICROS)
    _, want = y.orcl_scan(t["data"], t["offsets"], t["n_blocks"],
                          y.orcl_schema_from(t["schema"]), ospec,
                          collect_rows=True)
    assert len(want) > 0
    assert got == want


def _spec_pair(schema):
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(cc.READ_MICROS)
    spec.num_preds = 1
    spec.preds[0] = y.Pred(0, 0, y.PRED_GT, 70, None, 0)
    spec.num_aggs = 2
    spec.aggs[0] = y.Agg(y.AGG_COUNT_STAR, 0)
    spec.aggs[1] = y.Agg(y.AGG_SUM_INT64, 3)
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(cc.READ_MICROS)
    ospec.num_preds = 1
    ospec.preds[0] = y.OrclPred(0, 0, y.PRED_GT, 70, None, 0)
    ospec.num_aggs = 2
    ospec.aggs[0] = y.OrclAgg(y.AGG_COUNT_STAR, 0)
    ospec.aggs[1] = y.OrclAgg(y.AGG_SUM_INT64, 3)
    return spec, ospec


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_host_simulator_over_decompressed_blocks(key):
    """sim_scan over the host-decompressed file equals the oracle over the
    raw blocks (as test_sst_scan_parity_oracle, for compressed files)."""
    t = cc.tablets()[key[0]]
    entries = cc.corpus_entry(*key)
    sst, handles = cc.write_sst([(s, bt) for s, bt, _ in entries])
    offs, szs = y.sst_index(sst, verify=True)
    parts = [host_decode(sst[o:o + s], sst[o + s], len(raw), guard=False)
             for (o, s), (_, _, raw) in zip(zip(offs, szs), entries)]
    blocks = b"".join(parts)
    boffs = [0]
    for p in parts:
        boffs.append(boffs[-1] + len(p))
    buf = (C.c_uint8 * (len(blocks) + cc.SLACK)).from_buffer_copy(
        blocks + b"\0" * cc.SLACK)
    offarr = (C.c_uint64 * len(boffs))(*boffs)
    spec, ospec = _spec_pair(t["schema"])
    sres = y.sim_scan(spec, buf, offarr, len(parts))
    ores, _ = y.orcl_scan(t["data"], t["offsets"], t["n_blocks"],
                          y.orcl_schema_from(t["schema"]), ospec)
    assert ores.rows_matched > 0
    assert sres.rows_scanned == ores.rows_scanned
    assert sres.rows_matched == ores.rows_matched
    assert sres.aggs[0].value_i64 == ores.aggs[0].value_i64
    assert sres.aggs[1].value_i64 == ores.aggs[1].value_i64
