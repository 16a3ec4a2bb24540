"""Independent codecs, stream corpus and SST writer for the SST feed path.

Everything codec- and file-format-related in this module is written from the
public format descriptions alone and imports nothing from the code under
test:

  * ref_snappy_decode / ref_lz4_decode restate the Snappy raw format
    (google/snappy format_description.txt) and the LZ4 block format
    (lz4.org block format description) with rocksdb's varint32 raw-length
    framing. They raise CodecError on anything malformed and are THE
    reference: every stream an encoder here produces is decoded by them
    before it is shown to the product.
  * snappy_encode / lz4_encode produce full-format streams: every copy kind,
    every literal-length form, split and overlapping copies ("real" mode
    picks what the real compressors pick, "mix" mode picks at random among
    all legal forms).
  * census() counts the element kinds of a stream, so that a test can assert
    that the corpus holds what it is meant to hold.
  * write_sst() lays out a BlockBasedTable file (block trailers, empty
    metaindex block, index block, version-2 footer) from the format.
  * malformed() lists streams every decoder must reject.

Three helpers use the project, none of them the code under test: tablets()
and small_twin_blocks() build the raw blocks to compress with ybgpu.Builder,
exactly as the scan will later read them; oracle_rows() reads rows back
with the CPU oracle; harmless_flip() uses both to find a bit of a stored
block whose flip leaves the block well formed.

`python tests/codec_cases.py --dump FILE` writes the corpus and the malformed
list for the stand-alone sanitizer driver (csrc/codec_sim_main.cc).
"""
import functools
import random
import struct
import sys

SNAPPY, LZ4 = 1, 4          # block trailer type bytes
CODEC_NAMES = {SNAPPY: "snappy", LZ4: "lz4"}
MODES = ("real", "mix")
TABLETS = ("small", "big", "noise")
SLACK = 48                  # tail slack the feed path may read (finish_sst)

MAGIC = 0x88E241B785F4CFF7
FOOTER_LEN = 53
TRAILER_LEN = 5

# exact run lengths the LZ4 "mix" encoder aims for: the last value a nibble
# holds, the first extended one, and both sides of one and two 255 bytes
LZ4_LIT_TARGETS = (14, 15, 15 + 254, 15 + 255, 15 + 510)
LZ4_MATCH_TARGETS = (18, 19, 19 + 254, 19 + 255, 19 + 510)
LZ4_OFF_TARGETS = (1, 2, 3, 65535)


class CodecError(ValueError):
    pass


# ---- crc32c / mask (bytewise, independent of the C++ tables) ---------------

def _mk_tab():
    tab = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (0x82F63B78 ^ (c >> 1)) if (c & 1) else (c >> 1)
        tab.append(c)
    return tab


def _crc32c(data, crc=0):
    # Castagnoli, reflected poly 0x82F63B78 — bytewise, independent of the
    # C++ implementation under test
    tab = _crc32c.tab
    c = crc ^ 0xFFFFFFFF
    for b in data:
        c = tab[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


_crc32c.tab = _mk_tab()


def _mask(crc):
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def trailer(stored, btype):
    """[type | masked crc32c(contents + type)] of one stored block."""
    crc = _crc32c(bytes([btype]), _crc32c(stored))
    return bytes([btype]) + struct.pack("<I", _mask(crc))


# ---- varints ----------------------------------------------------------------

def uvarint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def read_uvarint32(s, ip=0):
    """(value, next position) of a varint32: at most 5 bytes, below 2**32."""
    v = 0
    for k in range(5):
        if ip >= len(s):
            raise CodecError("truncated varint")
        b = s[ip]
        ip += 1
        v |= (b & 0x7F) << (7 * k)
        if not b & 0x80:
            if v >> 32:
                raise CodecError("varint32 overflow")
            return v, ip
    raise CodecError("varint32 longer than 5 bytes")


# ---- reference decoders -----------------------------------------------------

def _copy_back(out, off, ln):
    """Append ln bytes starting off bytes back; overlap repeats the tail."""
    if off >= ln:
        start = len(out) - off
        out += out[start:start + ln]
    else:
        pat = bytes(out[-off:])
        out += (pat * (ln // off + 1))[:ln]


def ref_snappy_decode(stream):
    s = bytes(stream)
    n = len(s)
    ulen, ip = read_uvarint32(s)
    out = bytearray()
    while ip < n:
        tag = s[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            if ln > 60:
                nb = ln - 60
                if ip + nb > n:
                    raise CodecError("truncated literal length")
                ln = int.from_bytes(s[ip:ip + nb], "little") + 1
                ip += nb
            if ip + ln > n:
                raise CodecError("literal runs past the source")
            if len(out) + ln > ulen:
                raise CodecError("literal runs past the stated length")
            out += s[ip:ip + ln]
            ip += ln
            continue
        if kind == 1:
            ln = ((tag >> 2) & 7) + 4
            if ip + 1 > n:
                raise CodecError("truncated copy-1 operand")
            off = ((tag >> 5) << 8) | s[ip]
            ip += 1
        elif kind == 2:
            ln = (tag >> 2) + 1
            if ip + 2 > n:
                raise CodecError("truncated copy-2 operand")
            off = s[ip] | (s[ip + 1] << 8)
            ip += 2
        else:
            ln = (tag >> 2) + 1
            if ip + 4 > n:
                raise CodecError("truncated copy-4 operand")
            off = int.from_bytes(s[ip:ip + 4], "little")
            ip += 4
        if off == 0 or off > len(out):
            raise CodecError("copy offset outside the output")
        if len(out) + ln > ulen:
            raise CodecError("copy runs past the stated length")
        _copy_back(out, off, ln)
    if len(out) != ulen:
        raise CodecError("stream ends short of the stated length")
    return bytes(out)


def ref_lz4_decode(stream):
    """Stored LZ4 block: uvarint32(raw length) + LZ4 block data."""
    s = bytes(stream)
    n = len(s)
    ulen, ip = read_uvarint32(s)
    out = bytearray()
    while True:
        if ip >= n:
            raise CodecError("no final literal-only sequence")
        token = s[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    raise CodecError("truncated literal length")
                b = s[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        if ip + lit > n:
            raise CodecError("literals run past the source")
        if len(out) + lit > ulen:
            raise CodecError("literals run past the framed length")
        out += s[ip:ip + lit]
        ip += lit
        if ip == n:
            break  # the final sequence holds literals only
        if ip + 2 > n:
            raise CodecError("truncated match offset")
        off = s[ip] | (s[ip + 1] << 8)
        ip += 2
        if off == 0 or off > len(out):
            raise CodecError("match offset outside the output")
        ml = token & 15
        if ml == 15:
            while True:
                if ip >= n:
                    raise CodecError("truncated match length")
                b = s[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if len(out) + ml > ulen:
            raise CodecError("match runs past the framed length")
        _copy_back(out, off, ml)
    if len(out) != ulen:
        raise CodecError("output differs from the framed length")
    return bytes(out)


# ---- match finding shared by the encoders -----------------------------------

def _extend(d, a, b, limit):
    """Length of the match between d[a:] and d[b:] (a < b), given that the
    first 4 bytes agree, not reading d[limit:]."""
    ln = 4
    while b + ln < limit:
        step = min(128, limit - b - ln)
        if d[a + ln:a + ln + step] == d[b + ln:b + ln + step]:
            ln += step
            continue
        while d[a + ln] == d[b + ln]:
            ln += 1
        break
    return ln


# ---- Snappy encoder ---------------------------------------------------------

def _snappy_literal(out, chunk, nb=None):
    """One literal element; nb forces that many extra length bytes."""
    lm = len(chunk) - 1
    need = 0 if lm < 60 else (lm.bit_length() + 7) // 8
    if nb is None or nb < need:
        nb = need
    if nb == 0:
        out.append(lm << 2)
    else:
        out.append((59 + nb) << 2)
        out += lm.to_bytes(nb, "little")
    out += chunk


def _snappy_copy(out, kind, off, ln):
    if kind == 1:
        assert 4 <= ln <= 11 and off < 2048
        out.append(1 | ((ln - 4) << 2) | ((off >> 8) << 5))
        out.append(off & 0xFF)
    elif kind == 2:
        assert 1 <= ln <= 64 and off < 65536
        out.append(2 | ((ln - 1) << 2))
        out += struct.pack("<H", off)
    else:
        assert 1 <= ln <= 64 and off < (1 << 32)
        out.append(3 | ((ln - 1) << 2))
        out += struct.pack("<I", off)


def _snappy_copy_real(out, off, ln):
    """What real Snappy emits for one match: 64-byte pieces, then the
    smallest form that holds the rest (1-byte offset when off < 2048 and
    4 <= len <= 11); 4-byte offsets only above 65535."""
    wide = 3 if off > 65535 else 2
    while ln >= 68:
        _snappy_copy(out, wide, off, 64)
        ln -= 64
    if ln > 64:
        _snappy_copy(out, wide, off, 60)
        ln -= 60
    if wide == 2 and off < 2048 and 4 <= ln <= 11:
        _snappy_copy(out, 1, off, ln)
    else:
        _snappy_copy(out, wide, off, ln)


def _snappy_copy_mix(out, off, ln, rng):
    while ln:
        kinds = [3]
        if off < 65536:
            kinds.append(2)
        if off < 2048 and ln >= 4:
            kinds += [1, 1]
        kind = rng.choice(kinds)
        lo, hi = (4, min(11, ln)) if kind == 1 else (1, min(64, ln))
        piece = hi if rng.random() < 0.6 else rng.randint(lo, hi)
        _snappy_copy(out, kind, off, piece)
        ln -= piece


def snappy_encode(data, rng, mode, far=False):
    """Raw Snappy stream of data. far keeps the OLDEST candidate of a hash
    slot, so that offsets above 65535 really occur."""
    d = bytes(data)
    n = len(d)
    out = bytearray(uvarint(n))
    table = {}
    ip = lit = 0

    def flush(upto):
        pos = lit
        while pos < upto:
            if mode == "real":
                chunk, nb = d[pos:upto], None
            else:
                take = upto - pos
                if rng.random() < 0.5:
                    take = rng.randint(1, take)
                chunk = d[pos:pos + take]
                nb = rng.randint(1, 4) if rng.random() < 0.3 else None
            _snappy_literal(out, chunk, nb)
            pos += len(chunk)

    while ip + 4 <= n:
        key = d[ip:ip + 4]
        cand = table.get(key)
        if cand is None or not far:
            table[key] = ip
        if cand is None:
            ip += 1
            continue
        ln = _extend(d, cand, ip, n)    # may run into its own output
        flush(ip)
        if mode == "real":
            _snappy_copy_real(out, ip - cand, ln)
        else:
            _snappy_copy_mix(out, ip - cand, ln, rng)
        ip += ln
        lit = ip
    flush(n)
    return bytes(out)


# ---- LZ4 encoder ------------------------------------------------------------

def _lz4_sequence(out, lits, off, ml):
    """One sequence; ml == 0 is the final, literal-only one."""
    ln = len(lits)
    m = ml - 4 if ml else 0
    out.append((min(ln, 15) << 4) | min(m, 15))
    if ln >= 15:
        r = ln - 15
        out += b"\xff" * (r // 255)
        out.append(r % 255)
    out += lits
    if not ml:
        return
    out += struct.pack("<H", off)
    if m >= 15:
        r = m - 15
        out += b"\xff" * (r // 255)
        out.append(r % 255)


def lz4_encode(data, rng, mode):
    """Stored LZ4 block: uvarint32(len) + LZ4 block data."""
    d = bytes(data)
    n = len(d)
    out = bytearray(uvarint(n))
    table = {}
    real = mode == "real"
    # real LZ4 end conditions: the last match starts 12+ bytes before the
    # end and the last 5 bytes are literals; "mix" matches up to the end
    mflimit = n - 12 if real else n - 3
    matchlimit = n - 5 if real else n
    ip = anchor = 0
    want_lit = None            # literal run length this run aims for
    offs_left = list(LZ4_OFF_TARGETS)
    match_left = list(LZ4_MATCH_TARGETS)

    def pick_lit_target():
        if real or rng.random() >= 0.3:
            return None
        fit = [w for w in LZ4_LIT_TARGETS if anchor + w + 4 <= n]
        return rng.choice(fit) if fit else None

    while ip < mflimit:
        key = d[ip:ip + 4]
        cand = table.get(key)
        table[key] = ip
        if not real:
            # any valid match is legal: probe the offsets still wanted
            for o in offs_left:
                if ip >= o and d[ip - o:ip - o + 4] == key:
                    cand = ip - o
                    break
        if cand is None or ip - cand > 65535:
            ip += 1
            continue
        run = ip - anchor
        if want_lit is not None:
            if run < want_lit:
                ip += 1        # pass the match by: the run is still short
                continue
            want_lit = None    # reached (run == want_lit) or overshot
        off = ip - cand
        ml = _extend(d, cand, ip, matchlimit)
        exact = False
        if not real:
            if off in offs_left:
                offs_left.remove(off)
            # cut the match to the longest length still wanted in this block
            fit = [w for w in match_left if w <= ml]
            if fit and rng.random() < 0.7:
                ml = max(fit)
                match_left.remove(ml)
                exact = True
        lits = d[anchor:ip]
        if not real and not exact and ml >= 8 and rng.random() < 0.3:
            first = rng.randint(4, ml - 4)      # split: a zero-literal
            _lz4_sequence(out, lits, off, first)  # sequence follows
            _lz4_sequence(out, b"", off, ml - first)
        else:
            _lz4_sequence(out, lits, off, ml)
        ip += ml
        anchor = ip
        want_lit = pick_lit_target()
    _lz4_sequence(out, d[anchor:], 0, 0)   # token 0x00 when nothing is left
    return bytes(out)


# ---- census -----------------------------------------------------------------

SNAPPY_KEYS = ("copy1", "copy2", "copy4", "lit0", "lit1", "lit2", "lit3",
               "lit4", "off_eq_1", "off_lt_len", "off_ge_2048",
               "off_gt_65535")
LZ4_KEYS = ("lit_ext", "lit_ext_255", "match_ext", "match_ext_255",
            "zero_literal", "off_eq_1", "off_lt_mlen", "empty_final") + \
    tuple("lit_%d" % w for w in LZ4_LIT_TARGETS) + \
    tuple("match_%d" % w for w in LZ4_MATCH_TARGETS) + \
    tuple("off_%d" % w for w in LZ4_OFF_TARGETS if w != 1)


def census(stream, codec):
    """Element kinds of a VALID stream, as a dict of counts."""
    s = bytes(stream)
    n = len(s)
    if codec == SNAPPY:
        c = dict.fromkeys(SNAPPY_KEYS, 0)
        _, ip = read_uvarint32(s)
        while ip < n:
            tag = s[ip]
            ip += 1
            kind = tag & 3
            if kind == 0:
                ln = (tag >> 2) + 1
                nb = ln - 60 if ln > 60 else 0
                if nb:
                    ln = int.from_bytes(s[ip:ip + nb], "little") + 1
                c["lit%d" % nb] += 1
                ip += nb + ln
                continue
            if kind == 1:
                ln = ((tag >> 2) & 7) + 4
                off = ((tag >> 5) << 8) | s[ip]
                ip += 1
                c["copy1"] += 1
            else:
                ln = (tag >> 2) + 1
                width = 2 if kind == 2 else 4
                off = int.from_bytes(s[ip:ip + width], "little")
                ip += width
                c["copy%d" % width] += 1
            c["off_eq_1"] += off == 1
            c["off_lt_len"] += off < ln
            c["off_ge_2048"] += off >= 2048
            c["off_gt_65535"] += off > 65535
        return c
    c = dict.fromkeys(LZ4_KEYS, 0)
    _, ip = read_uvarint32(s)
    while True:
        token = s[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            c["lit_ext"] += 1
            while True:
                b = s[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
                c["lit_ext_255"] += 1
        ip += lit
        if ip == n:
            c["empty_final"] += lit == 0
            return c
        if lit in LZ4_LIT_TARGETS:
            c["lit_%d" % lit] += 1
        c["zero_literal"] += lit == 0
        off = s[ip] | (s[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            c["match_ext"] += 1
            while True:
                b = s[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
                c["match_ext_255"] += 1
        ml += 4
        if ml in LZ4_MATCH_TARGETS:
            c["match_%d" % ml] += 1
        if off in LZ4_OFF_TARGETS and off != 1:
            c["off_%d" % off] += 1
        c["off_eq_1"] += off == 1
        c["off_lt_mlen"] += off < ml


def census_sum(entries, codec):
    total = dict.fromkeys(SNAPPY_KEYS if codec == SNAPPY else LZ4_KEYS, 0)
    for stored, btype, _raw in entries:
        if btype != codec:
            continue
        for k, v in census(stored, codec).items():
            total[k] += v
    return total


# ---- SST writer -------------------------------------------------------------

def write_sst(blocks):
    """BlockBasedTable file of the (stored_bytes, type) data blocks, from the
    format alone: block trailers, an empty metaindex block, an index block
    with restart interval 1 and dummy 8-byte keys whose values are the
    BlockHandles, and a version-2 footer (rocksdb table/format.cc). Returns
    (file_bytes, handles) with handles = [(offset, size)]."""
    out = bytearray()
    handles = []
    for stored, btype in blocks:
        handles.append((len(out), len(stored)))
        out += stored
        out += trailer(stored, btype)
    # metaindex: no entries, one restart point at 0
    meta = struct.pack("<II", 0, 1)
    meta_h = (len(out), len(meta))
    out += meta + trailer(meta, 0)
    index = bytearray()
    restarts = []
    for i, (off, size) in enumerate(handles):
        restarts.append(len(index))
        value = uvarint(off) + uvarint(size)
        index += uvarint(0) + uvarint(8) + uvarint(len(value))
        index += struct.pack(">Q", i) + value
    for r in restarts:
        index += struct.pack("<I", r)
    index += struct.pack("<I", len(restarts))
    index = bytes(index)
    index_h = (len(out), len(index))
    out += index + trailer(index, 0)
    footer = bytearray([1])     # kCRC32c
    footer += uvarint(meta_h[0]) + uvarint(meta_h[1])
    footer += uvarint(index_h[0]) + uvarint(index_h[1])
    footer += b"\0" * (41 - len(footer))
    footer += struct.pack("<III", 2, MAGIC & 0xFFFFFFFF, MAGIC >> 32)
    assert len(footer) == FOOTER_LEN
    out += footer
    return bytes(out), handles


def sst_buffer(file_bytes):
    """(pointer, size) over a copy of the file with the tail slack
    Builder.finish_sst leaves behind the file."""
    import ctypes as C
    buf = (C.c_uint8 * (len(file_bytes) + SLACK)).from_buffer_copy(
        bytes(file_bytes) + b"\0" * SLACK)
    return C.cast(buf, C.POINTER(C.c_uint8)), len(file_bytes)


def refresh_trailer(sst, handle, btype=None):
    """Recompute the trailer CRC of one block in place (bytearray)."""
    off, size = handle
    if btype is None:
        btype = sst[off + size]
    sst[off + size:off + size + TRAILER_LEN] = trailer(
        bytes(sst[off:off + size]), btype)


FLIP_TYPE = {0: 1, 1: 0, 4: 0}   # another type the parser accepts


def crc_flips(file_bytes, handles, count=4):
    """One-byte corruptions the trailer check must catch: for `count` blocks
    that cover the four residues of (size + 1) % 4, the first byte, each of
    the last three bytes, the trailer type byte (to another accepted type)
    and each CRC byte. Returns (attacked block indices, [(name, position,
    xor mask)])."""
    picked, seen, seen_align = [], set(), set()
    for distinct_align in (True, False):   # prefer distinct offset % 8 too
        for i, (off, size) in enumerate(handles):
            if len(picked) == count:
                break
            if size < 4 or i in picked or (size + 1) % 4 in seen:
                continue
            if distinct_align and off % 8 in seen_align:
                continue
            seen.add((size + 1) % 4)
            seen_align.add(off % 8)
            picked.append(i)
    flips = []
    for i in picked:
        off, size = handles[i]
        flips.append(("b%d_first" % i, off, 0x01))
        for k in (1, 2, 3):
            flips.append(("b%d_last%d" % (i, k), off + size - k, 0x01))
        t = file_bytes[off + size]
        flips.append(("b%d_type" % i, off + size, t ^ FLIP_TYPE[t]))
        for k in range(4):
            flips.append(("b%d_crc%d" % (i, k), off + size + 1 + k, 0x10))
    return picked, flips


def oracle_rows(schema, blocks):
    """Every row of a list of raw blocks, from the CPU oracle."""
    import ctypes as C
    import ybgpu as y
    joined = b"".join(blocks)
    buf = (C.c_uint8 * (len(joined) + SLACK)).from_buffer_copy(
        joined + b"\0" * SLACK)
    offs = [0]
    for b in blocks:
        offs.append(offs[-1] + len(b))
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(READ_MICROS)
    _, rows = y.orcl_scan(C.cast(buf, C.POINTER(C.c_uint8)),
                          (C.c_uint64 * len(offs))(*offs), len(blocks),
                          y.orcl_schema_from(schema), ospec,
                          collect_rows=True)
    return rows


def harmless_flip(schema, entries, i):
    """A one-bit flip inside stored block i after which the block is still
    well formed: the reference decodes it to a block of the same length that
    differs in one byte, and the oracle reads the same rows from it with one
    value changed. Returns (position in the stored block, the raw blocks
    after the flip). With its CRC recomputed, such a file must feed."""
    stored, btype, raw = entries[i]
    decode = ref_snappy_decode if btype == SNAPPY else ref_lz4_decode
    blocks = [r for _, _, r in entries]
    lo, hi = max(0, i - 1), min(len(blocks), i + 2)
    want = oracle_rows(schema, blocks[lo:hi])
    # only bytes that the builder itself changes when every value has its
    # lowest bit flipped: the block stays one the builder could have written
    twin = small_twin_blocks()[i]
    assert len(twin) == len(raw)
    for pos in range(len(stored) // 2, len(stored)):
        bad = bytearray(stored)
        bad[pos] ^= 0x01
        try:
            out = decode(bytes(bad))
        except CodecError:
            continue
        if len(out) != len(raw):
            continue
        diff = [p for p in range(len(raw)) if out[p] != raw[p]]
        if len(diff) != 1 or out[diff[0]] != twin[diff[0]]:
            continue
        got = oracle_rows(schema, blocks[lo:i] + [out] + blocks[i + 1:hi])
        if len(got) == len(want) and \
                [k for k, _ in got] == [k for k, _ in want] and \
                sum(g != w for g, w in zip(got, want)) == 1:
            return pos, blocks[:i] + [out] + blocks[i + 1:]
    raise AssertionError("no harmless flip in block %d" % i)


# ---- tablets ----------------------------------------------------------------

_KEEP = []
READ_MICROS = 1_700_000_000_000_000


def _finish(name, schema, b):
    import ctypes as C
    data, offsets, n_blocks, total, n_entries = b.finish()
    _KEEP.append(b)
    raw = bytes(C.cast(data, C.POINTER(C.c_uint8 * total)).contents)
    offs = [offsets[i] for i in range(n_blocks + 1)]
    return {"name": name, "schema": schema, "data": data, "offsets": offsets,
            "n_blocks": n_blocks, "total": total, "n_entries": n_entries,
            "blocks": [raw[offs[i]:offs[i + 1]] for i in range(n_blocks)]}


def _small(schema, flip):
    import ybgpu as y
    b = y.Builder(schema, block_size=512)
    for r in range(3300):
        b.add_packed_row(1000 + r,
                         [(y.T_INT64, (r * 7 + c) ^ flip) for c in range(4)],
                         hash_=r // 64, key_datums=(r,), packed_version=2)
    return _finish("small", schema, b)


@functools.lru_cache(maxsize=None)
def small_twin_blocks():
    """The small tablet with the lowest bit of every value flipped: same
    block sizes, and it differs from the small tablet exactly in the lowest
    byte of each value."""
    return _small(tablets()["small"]["schema"], 1)["blocks"]


@functools.lru_cache(maxsize=None)
def tablets():
    """The raw blocks to compress, smallest shapes that reach every branch:
    small — 4 INT64 columns of r*7+c in 512-byte blocks: more than 256
            blocks (a second workgroup of both kernels), 2-byte preambles;
    big   — the same plus a string column in 128 KB blocks: 3-byte
            preambles, long byte runs, and a random value that recurs more
            than 65535 bytes later inside a block (far copy-4);
    noise — random 64-bit values in two rows out of three: blocks that do
            not shrink sit between blocks that do."""
    import ybgpu as y
    from snapshot_string_cases import edge_value
    ints = [(10 + i, y.T_INT64, 1) for i in range(4)]
    out = {}

    schema = y.make_schema([y.KT_INT64], ints)
    out["small"] = _small(schema, 0)

    rng = random.Random(20240)
    far = bytes(rng.randrange(256) for _ in range(48))
    schema = y.make_schema([y.KT_INT64], ints + [(14, y.T_STRING, 1)])
    b = y.Builder(schema, block_size=131072)
    for r in range(3000):
        if r % 1500 in (3, 1203):
            s = far                         # recurs ~90 KB later
        elif r % 97 == 11:
            s = bytes([65 + r % 7]) * 1400  # long runs, offsets 1, 2, 3
        else:
            s = edge_value(r)
        b.add_packed_row(1000 + r,
                         [(y.T_INT64, r * 7 + c) for c in range(4)] +
                         [(y.T_STRING, s)],
                         hash_=r // 64, key_datums=(r,), packed_version=2)
    out["big"] = _finish("big", schema, b)

    schema = y.make_schema([y.KT_INT64], ints + [(14, y.T_STRING, 1)])
    b = y.Builder(schema, block_size=512)
    for r in range(900):
        if (r // 10) % 3:
            vals = [rng.getrandbits(64) for _ in range(4)]
        else:
            vals = [r * 7 + c for c in range(4)]
        # NULLs and a string of 0 .. 10 bytes make the rows, hence the
        # blocks, differ in length byte by byte
        vals = [None if rng.random() < 0.15 else v for v in vals]
        b.add_packed_row(1000 + r, [(y.T_INT64, v) for v in vals] +
                         [(y.T_STRING, edge_value(r)[:rng.randrange(11)]
                           if edge_value(r) is not None else None)],
                         hash_=r // 64, key_datums=(r,), packed_version=2)
    out["noise"] = _finish("noise", schema, b)
    return out


def _seed(*parts):
    return sum((i + 1) * 7919 * sum(str(p).encode()) for i, p in
               enumerate(parts))


def encode_block(raw, codec, mode, rng, far=False):
    if codec == SNAPPY:
        stored = snappy_encode(raw, rng, mode, far=far)
        back = ref_snappy_decode(stored)
    else:
        stored = lz4_encode(raw, rng, mode)
        back = ref_lz4_decode(stored)
    assert back == raw, "encoder output fails the reference decoder"
    return stored


@functools.lru_cache(maxsize=None)
def corpus_entry(tablet, codec, mode):
    """[(stored_bytes, type, raw_block)] of one tablet. In the noise tablet
    every third block, and every block that does not shrink, is type 0."""
    rng = random.Random(_seed(tablet, codec, mode))
    out = []
    for i, raw in enumerate(tablets()[tablet]["blocks"]):
        stored = encode_block(raw, codec, mode, rng,
                              far=(tablet == "big" and mode == "mix"))
        if tablet == "noise" and (i % 3 == 2 or len(stored) >= len(raw)):
            out.append((raw, 0, raw))
        else:
            out.append((stored, codec, raw))
    return out


def corpus():
    return {(t, c, m): corpus_entry(t, c, m)
            for t in TABLETS for c in (SNAPPY, LZ4) for m in MODES}


@functools.lru_cache(maxsize=None)
def alternating_entry():
    """The noise tablet with block i stored as type (0, 1, 4)[i % 3]: all
    three branches of the decompression kernel in one file."""
    rng = random.Random(_seed("alternating"))
    out = []
    for i, raw in enumerate(tablets()["noise"]["blocks"]):
        codec = (0, SNAPPY, LZ4)[i % 3]
        if codec == 0:
            out.append((raw, 0, raw))
        else:
            out.append((encode_block(raw, codec, "mix", rng), codec, raw))
    return out


# ---- malformed streams ------------------------------------------------------

def _lit(chunk):
    out = bytearray()
    _snappy_literal(out, chunk)
    return bytes(out)


def snappy_ulen(stream):
    return read_uvarint32(stream)[0]


def malformed():
    """[(name, codec, stream, cap)] every decoder must reject when called
    with capacity cap. LZ4 streams are stored blocks framed with
    uvarint32(cap)."""
    c2 = lambda ln, off: bytes([2 | ((ln - 1) << 2)]) + struct.pack("<H", off)
    c4 = lambda ln, off: bytes([3 | ((ln - 1) << 2)]) + struct.pack("<I", off)
    c1 = lambda ln, off: bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5),
                                off & 0xFF])
    abcd = _lit(b"abcd")
    S = SNAPPY
    cases = [
        ("empty", S, b"", 16),
        ("truncated_preamble", S, b"\x80", 16),
        ("truncated_preamble_2", S, b"\xff\xff", 16),
        ("preamble_6_bytes", S, b"\x80\x80\x80\x80\x80\x00" + abcd, 16),
        # five bytes, value 2**32 + 4: above what a varint32 holds. (The
        # host decoder rejects it at this capacity either way; the feed
        # path, which sizes the slot from the preamble, is where it counts.)
        ("preamble_above_32_bits", S, b"\x84\x80\x80\x80\x10" + abcd, 16),
        # the stated length is one more than the capacity (and than the
        # elements give, so the stream is malformed at any capacity)
        ("ulen_gt_cap", S, uvarint(17) + _lit(b"x" * 16), 16),
        ("literal_past_source", S, uvarint(10) + bytes([9 << 2]) + b"12345",
         64),
        ("literal_past_ulen", S, uvarint(5) + _lit(b"123456"), 64),
        ("long_literal_past_ulen", S, uvarint(70) + _lit(b"y" * 71), 128),
        ("truncated_literal_length", S,
         uvarint(100) + bytes([61 << 2]) + b"\x63", 128),
        ("literal_length_ffffffff", S,
         uvarint(10) + bytes([63 << 2]) + b"\xff\xff\xff\xff" + b"0123456789",
         64),
        ("copy1_offset_0", S, uvarint(8) + abcd + c1(4, 0), 64),
        ("copy2_offset_0", S, uvarint(8) + abcd + c2(4, 0), 64),
        ("copy4_offset_0", S, uvarint(8) + abcd + c4(4, 0), 64),
        ("copy1_offset_op_plus_1", S, uvarint(8) + abcd + c1(4, 5), 64),
        ("copy2_offset_op_plus_1", S, uvarint(8) + abcd + c2(4, 5), 64),
        ("copy4_offset_op_plus_1", S, uvarint(8) + abcd + c4(4, 5), 64),
        ("copy_first_element", S, uvarint(4) + c1(4, 1), 64),
        ("copy2_first_element", S, uvarint(4) + c2(4, 1), 64),
        ("copy_past_ulen", S, uvarint(6) + abcd + c2(4, 4), 64),
        ("copy1_past_ulen", S, uvarint(14) + abcd + c1(11, 1), 64),
        ("copy1_operand_cut", S, uvarint(8) + abcd + c1(4, 4)[:1], 64),
        ("copy2_operand_cut", S, uvarint(8) + abcd + c2(4, 4)[:2], 64),
        ("copy4_operand_cut", S, uvarint(8) + abcd + c4(4, 4)[:4], 64),
        ("copy4_offset_ffffffff", S, uvarint(8) + abcd + c4(4, 0xFFFFFFFF),
         64),
        ("ends_short_of_ulen", S, uvarint(10) + abcd, 64),
        ("element_beyond_ulen", S, uvarint(4) + abcd + _lit(b"z"), 64),
        ("copy_beyond_ulen", S, uvarint(4) + abcd + c2(1, 1), 64),
    ]

    def lz(cap, body):
        return uvarint(cap) + body

    L = LZ4
    cases += [
        ("lz4_truncated_literal_ext", L, lz(300, b"\xf0\xff"), 300),
        ("lz4_literal_past_source", L, lz(5, b"\x50abc"), 5),
        ("lz4_offset_0", L, lz(8, b"\x40abcd\x00\x00\x00"), 8),
        ("lz4_offset_op_plus_1", L, lz(8, b"\x40abcd\x05\x00\x00"), 8),
        ("lz4_offset_1_byte", L, lz(8, b"\x40abcd\x01"), 8),
        ("lz4_truncated_match_ext", L, lz(300, b"\x4fabcd\x01\x00\xff"), 300),
        ("lz4_match_past_cap", L, lz(10, b"\x4fabcd\x01\x00\x00\x00"), 10),
        ("lz4_literal_past_cap", L, lz(3, b"\x40abcd"), 3),
        ("lz4_one_byte_short", L, lz(10, b"\x90123456789"), 10),
        ("lz4_one_byte_long", L, lz(10, b"\xb00123456789a"), 10),
        ("lz4_match_one_byte_long", L, lz(10, b"\x43abcd\x04\x00\x00"), 10),
        # the right number of bytes, but the block ends on a match: no
        # final literal-only sequence
        ("lz4_ends_on_match", L, lz(8, b"\x40abcd\x04\x00"), 8),
    ]
    return cases


# ---- dump for the stand-alone sanitizer driver ------------------------------

def dump(path):
    """Records (codec u8, expect i64, cap u64, n u64, n stream bytes,
    expect output bytes when expect >= 0) after a u32 record count. For a
    corpus stream cap == expect == the raw length; for a malformed one
    expect is -1."""
    recs = []
    for key, entries in sorted(corpus().items()):
        for stored, btype, raw in entries:
            if btype:
                recs.append((btype, len(raw), len(raw), stored, raw))
    for stored, btype, raw in alternating_entry():
        if btype:
            recs.append((btype, len(raw), len(raw), stored, raw))
    for _name, codec, stream, cap in malformed():
        recs.append((codec, -1, cap, stream, b""))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for codec, expect, cap, stream, want in recs:
            f.write(struct.pack("<BqQQ", codec, expect, cap, len(stream)))
            f.write(stream)
            f.write(want)
    return len(recs)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        import os
        sys.path.insert(0, os.path.join(os.path.dirname(
            os.path.abspath(__file__)), ".."))
        print("%d records" % dump(sys.argv[2]))
    else:
        sys.exit("usage: codec_cases.py --dump FILE")
