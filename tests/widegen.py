"""A plain-Python model of compress_integer / decompress_integer for a signed
W-byte integer, W in {8, 16, 32} (`impl IntegerType for i64 / i128 / i256`,
compression/integer/traits.rs:30-39): whole flat pages, validity prefix
included.  Values are Python ints.  The oracle's library knows widths 1 to 8
only, so the wide tests bring this model; test_wide_model_cpu.py pins it to
the oracle byte for byte at W = 8.

What is not width-specific comes from the oracle: the Basic codecs
(common_compress / common_decompress), the roaring bitmap, the validity
prefix and Dict's u32 index stream (oracle.compress / decompress on a uint32
array, its sampler started at this page's current state).

The sampler is the deterministic splitmix64 of the engine's host encoder
(one word of state) standing in for the reference's thread_rng; Freq's top
value breaks ties by first occurrence where the reference follows HashMap
order.

Also here: builders that lay a page out with the codec the caller names, so
tests can make pages no writer would choose, and a reader that classifies
malformed pages as the oracle's does (OutOfSpec / Io / Codec)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

NONE, LZ4, ZSTD, SNAPPY = 0, 1, 2, 3
RLE, DICT, ONE_VALUE, FREQ, BITPACKING, DELTA_BITPACKING, PATAS = 10, 11, 12, 13, 14, 15, 16
E_OUT_OF_SPEC, E_IO, E_CODEC = 1, 3, 4
M64 = (1 << 64) - 1


class Malformed(Exception):
    """A page the reference cannot read; code as the oracle's status."""

    def __init__(self, code: int, what: str = ""):
        super().__init__(f"{what}: status {code}")
        self.code = code


def to_bytes(v: int, W: int) -> bytes:
    """Little-endian two's complement, W bytes (Arrow's decimal buffers)."""
    return (v & ((1 << (8 * W)) - 1)).to_bytes(W, "little")


def from_bytes(b: bytes) -> int:
    return int.from_bytes(b, "little", signed=True)


def pack(vals, W: int) -> bytes:
    return b"".join(to_bytes(int(v), W) for v in vals)


def unpack(raw: bytes, W: int):
    return [from_bytes(raw[i:i + W]) for i in range(0, len(raw), W)]


def as_array(vals, W: int) -> np.ndarray:
    """The values as the numpy array the engine's writer takes (int64 or V16 / V32)."""
    raw = np.frombuffer(pack(vals, W), np.uint8)
    return raw.view(np.int64) if W == 8 else raw.view(f"V{W}")


def as_i64(v: int) -> int:
    """IntegerType::as_i64 (traits.rs:30-39): `as i64`, the low 64 bits."""
    x = v & M64
    return x - (1 << 64) if x >> 63 else x


def u32(x: int) -> bytes:
    return int(x).to_bytes(4, "little")


class Rng:
    """splitmix64, one word of state (the host encoder's seeded sampler)."""

    def __init__(self, seed: int):
        self.s = seed & M64

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)


class Opts:
    """The fields of oracle.WriteOptions (write/common.rs:37-45 + forced codec)."""

    def __init__(self, o=None):
        o = o if o is not None else O.WriteOptions.make()
        self.default_codec, self.has_ratio, self.ratio = int(o.default_codec), bool(o.has_ratio), float(o.ratio)
        self.forbidden, self.forced, self.seed = int(o.forbidden_mask), int(o.forced_codec), int(o.seed)

    def forbid(self, codec: int) -> "Opts":
        r = Opts.__new__(Opts)
        r.__dict__.update(self.__dict__)
        r.forbidden |= 1 << codec
        return r

    def oracle(self, seed: int) -> O.WriteOptions:
        return O.WriteOptions(self.default_codec, int(self.has_ratio), self.ratio, self.forbidden, self.forced, seed)


_DEFAULT = None


def _dflt() -> Opts:
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Opts(O.WriteOptions.make())
        _DEFAULT.forced = -1
    return _DEFAULT


def _ok(valid, i) -> bool:
    return valid is None or bool(valid[i])


class Stats:
    """gen_stats (integer/mod.rs:179-229): counts, min and max run over every
    slot, null ones included; is_sorted over the valid ones, from T::default()."""

    def __init__(self, vals, valid, W):
        n = len(vals)
        self.tuple_count, self.total_bytes = n, n * W
        self.null_count = sum(1 for i in range(n) if not _ok(valid, i))
        self.is_sorted = True
        self.counts, self.first = {}, {}
        last = 0
        self.min = self.max = vals[0] if n else 0
        for i, v in enumerate(vals):
            if _ok(valid, i):
                if v < last:
                    self.is_sorted = False
                last = v
            if v in self.counts:
                self.counts[v] += 1
            else:
                self.counts[v] = 1
                self.first[v] = i
            if v > self.max:
                self.max = v
            elif v < self.min:
                self.min = v
        self.unique_count = len(self.counts)

    def top(self):
        """(count, first row) of the most frequent value, ties to the first occurrence."""
        best, bf = 0, None
        for v, c in self.counts.items():
            f = self.first[v]
            if c > best or (c == best and f < bf):
                best, bf = c, f
        return best, bf


# ---- codec bodies -----------------------------------------------------------
def rle_body(vals, valid, W) -> bytes:
    """RLE::compress (rle.rs:64-104): [u32 count][T value] per run; null slots extend the run."""
    out, seen, last, all_null = [], 0, 0, True
    for i, v in enumerate(vals):
        if _ok(valid, i):
            if all_null:
                all_null, last, seen = False, v, seen + 1
            elif last != v:
                out.append(u32(seen) + to_bytes(last, W))
                last, seen = v, 1
            else:
                seen += 1
        else:
            seen += 1
    if seen:
        out.append(u32(seen) + to_bytes(last, W))
    return b"".join(out)


def one_value_body(vals, valid, W) -> bytes:
    """OneValue (one_value.rs:63-75): the first valid value, else T::default()."""
    for i, v in enumerate(vals):
        if _ok(valid, i):
            return to_bytes(v, W)
    return to_bytes(0, W)


def dict_body(vals, valid, W, opt: Opts, rng: Rng) -> bytes:
    """Dict::compress (dict.rs:34-73): the u32 index stream through
    compress_integer::<u32> with Dict forbidden, then u32 k and k plain
    entries.  A null slot repeats the index before it (slot 0: T::default())."""
    ids, sets, idx = {}, [], []
    for i, v in enumerate(vals):
        if not _ok(valid, i):
            if i > 0:
                idx.append(idx[-1])
                continue
            v = 0
        if v not in ids:
            ids[v] = len(sets)
            sets.append(v)
        idx.append(ids[v])
    stream = O.compress(np.asarray(idx, np.uint32), None, opt.forbid(DICT).oracle(rng.s))
    return stream + u32(len(sets)) + pack(sets, W)


def freq_body(vals, valid, W, st: Stats, opt: Opts, rng: Rng) -> bytes:
    """Freq::compress (freq.rs:34-86): T top, u32 len, the roaring bitmap of
    the exception rows, then the exceptions through compress_integer::<T> with
    Freq forbidden."""
    top_null = st.null_count / st.tuple_count >= 0.9
    top = 0 if top_null else vals[st.top()[1]]
    pos = [i for i, v in enumerate(vals) if _ok(valid, i) and (top_null or v != top)]
    bm = O.roaring_encode(np.asarray(pos, np.uint32))
    return to_bytes(top, W) + u32(len(bm)) + bm + compress_stream([vals[i] for i in pos], None, W, opt.forbid(FREQ), rng)


def _extend(codec, vals, valid, W, st, opt, rng) -> bytes:
    if codec == RLE:
        return rle_body(vals, valid, W)
    if codec == ONE_VALUE:
        return one_value_body(vals, valid, W)
    if codec == DICT:
        return dict_body(vals, valid, W, opt, rng)
    if codec == FREQ:
        return freq_body(vals, valid, W, st, opt, rng)
    raise ValueError(codec)  # Bitpacking / DeltaBitpacking: size_of::<T>() == 4 only (bp.rs:92-100)


def _sample_ratio(codec, vals, valid, W, full: Stats, rng: Rng) -> float:
    """compress_sample_ratio (integer/mod.rs:310-347): ten windows of 64 rows,
    T::default() under the null slots of the rebuilt sample."""
    SC, SS, n = 10, 64, len(vals)
    if n // SC <= SS:
        size = len(_extend(codec, vals, valid, W, full, _dflt(), rng))
        return full.total_bytes / size if size else float("nan")  # (an empty stream: 0 / 0, never chosen)
    sep, rem = n // SC, n % SC
    sv, sb = [], [] if valid is not None else None
    for k in range(SC):
        range_end = (sep + rem if k == SC - 1 else sep) - SS
        begin = k * sep + rng.next() % range_end
        for j in range(begin, begin + SS):
            ok = _ok(valid, j)
            sv.append(vals[j] if ok else 0)
            if sb is not None:
                sb.append(ok)
    st = Stats(sv, sb, W)
    return st.total_bytes / len(_extend(codec, sv, sb, W, st, _dflt(), rng))


def _ratio(codec, vals, valid, W, s: Stats, rng: Rng) -> float:
    if codec == ONE_VALUE:
        return float(s.tuple_count) if s.unique_count <= 1 else 0.0
    if codec == FREQ:  # freq.rs:129-151; as_i64 truncates the maximum (freq.rs:146)
        if s.unique_count <= 1:
            return 0.0
        if s.null_count / s.tuple_count >= 0.9:
            return float(s.tuple_count - 1)
        if s.top()[0] / s.tuple_count >= 0.9 and as_i64(s.max) >= 256:
            return float(s.tuple_count - 1)
        return 0.0
    if codec == DICT:  # dict.rs:105-120
        if s.unique_count * 3 >= s.tuple_count:
            return 0.0
        after = s.unique_count * W + s.tuple_count * (s.unique_count.bit_length() // 8) + s.tuple_count * 2 // 128
        return s.total_bytes / after
    if codec == RLE:
        return _sample_ratio(RLE, vals, valid, W, s, rng)
    return 0.0  # Bitpacking / DeltaBitpacking: ratio 0 unless size_of::<T>() == 4 (bp.rs:92-100, delta_bp.rs:97-105)


def _choose(vals, valid, W, s: Stats, opt: Opts, rng: Rng) -> int:
    """choose_compressor (integer/mod.rs:231-308); a forced Bitpacking is ignored at these widths."""
    if opt.forced >= 0 and not (opt.forbidden >> opt.forced) & 1 and opt.forced in (FREQ, DICT, RLE):
        return opt.forced
    result = opt.default_codec
    if not opt.has_ratio:
        return result
    maxr = opt.ratio
    for c in (ONE_VALUE, FREQ, DICT, RLE, BITPACKING, DELTA_BITPACKING):
        if (opt.forbidden >> c) & 1:
            continue
        r = _ratio(c, vals, valid, W, s, rng)
        if r > maxr:
            maxr, result = r, c
            if r == float(s.tuple_count):
                break
    return result


def stream(codec: int, body: bytes, n: int, W: int) -> bytes:
    """[codec u8][csize u32][usize u32][body], usize = n * W (integer/mod.rs:49-63)."""
    return bytes([codec]) + u32(len(body)) + u32((n * W) & 0xFFFFFFFF) + body


def compress_stream(vals, valid, W: int, opt: Opts, rng: Rng) -> bytes:
    """compress_integer (integer/mod.rs:35-70)."""
    vals = [int(v) for v in vals]
    s = Stats(vals, valid, W)
    codec = _choose(vals, valid, W, s, opt, rng)
    body = O.common_compress(codec, pack(vals, W)) if codec <= SNAPPY else _extend(codec, vals, valid, W, s, opt, rng)
    return stream(codec, body, len(vals), W)


def write_page(vals, valid=None, nullable=False, opts=None, W: int = 16, seed=None) -> bytes:
    """write_simple (serialize.rs:52-132): the validity prefix, then the value stream."""
    opt = Opts(opts)
    rng = Rng(opt.seed if seed is None else seed)
    pre = b""
    if nullable:
        pre = O.write_validity(np.ones(len(vals), bool) if valid is None else np.asarray(valid, bool))
    return pre + compress_stream(vals, valid, W, opt, rng)


# ---- builders: pages with the codec the caller names -------------------------
def none_stream(vals, W):
    return stream(NONE, pack(vals, W), len(vals), W)


def basic_stream(codec, vals, W):
    return stream(codec, O.common_compress(codec, pack(vals, W)), len(vals), W)


def one_value_stream(v, n, W):
    return stream(ONE_VALUE, to_bytes(v, W), n, W)


def rle_stream(runs, n, W):
    """runs: [(count, value)]."""
    return stream(RLE, b"".join(u32(c) + to_bytes(v, W) for c, v in runs), n, W)


def runs_of(vals):
    runs = []
    for v in vals:
        if runs and runs[-1][1] == v:
            runs[-1][0] += 1
        else:
            runs.append([1, v])
    return [(c, v) for c, v in runs]


def index_stream(codec, idx) -> bytes:
    """A u32 stream under the named codec (Dict's indices)."""
    idx = np.asarray(idx, np.uint32)
    n = len(idx)
    if codec in (NONE, LZ4, ZSTD, SNAPPY):
        return stream(codec, O.common_compress(codec, idx.tobytes()), n, 4)
    if codec == RLE:
        return rle_stream(runs_of([int(x) for x in idx]), n, 4)
    if codec in (BITPACKING, DELTA_BITPACKING):  # bp.rs:37-65, delta_bp.rs:37-67: whole 128-value blocks
        assert n % 128 == 0
        body, initial = b"", 0
        for b0 in range(0, n, 128):
            blk = idx[b0:b0 + 128]
            b = O.bp4x_num_bits(blk)
            body += bytes([b]) + (O.bp4x_pack(blk, b, initial) if codec == DELTA_BITPACKING else O.bp4x_pack(blk, b))
            initial = int(blk[127])
        return stream(codec, body, n, 4)
    raise ValueError(codec)


def dict_stream(idx_stream: bytes, entries, n, W, k=None, entry_bytes=None):
    body = idx_stream + u32(len(entries) if k is None else k) + (pack(entries, W) if entry_bytes is None else entry_bytes)
    return stream(DICT, body, n, W)


def dictionary(vals):
    """(indices, entries) in first-occurrence order."""
    ids, sets, idx = {}, [], []
    for v in vals:
        if v not in ids:
            ids[v] = len(sets)
            sets.append(v)
        idx.append(ids[v])
    return idx, sets


def freq_stream(top_bytes: bytes, positions, exc_stream: bytes, n, W, bitmap=None):
    bm = O.roaring_encode(np.asarray(positions, np.uint32)) if bitmap is None else bitmap
    return stream(FREQ, top_bytes + u32(len(bm)) + bm + exc_stream, n, W)


def freq_split(vals, top):
    pos = [i for i, v in enumerate(vals) if v != top]
    return pos, [vals[i] for i in pos]


def page(value_stream: bytes, valid=None, nullable=False, n=None) -> bytes:
    if not nullable:
        return value_stream
    return O.write_validity(np.ones(n, bool) if valid is None else np.asarray(valid, bool)) + value_stream


# ---- reader -----------------------------------------------------------------
def _header(buf: bytes, pos: int):
    if pos + 9 > len(buf):
        raise Malformed(E_IO, "stream header")
    codec, csize = buf[pos], int.from_bytes(buf[pos + 1:pos + 5], "little")
    pos += 9
    if pos + csize > len(buf):
        raise Malformed(E_IO, "stream body")
    return codec, csize, pos


def _oracle_call(f, *a):
    try:
        return f(*a)
    except O.OracleError as e:
        raise Malformed(e.code, "oracle") from None


def decompress_stream(buf: bytes, pos: int, W: int, length: int):
    """decompress_integer (integer/mod.rs:72-117) -> (length * W raw bytes, new pos)."""
    codec, csize, pos = _header(buf, pos)
    body = buf[pos:pos + csize]
    if codec in (NONE, LZ4, ZSTD, SNAPPY):
        out = _oracle_call(O.common_decompress, codec, body, length * W)
    elif codec == RLE:  # rle.rs:106-134: stops once `length` values are out; must land on it (array/integer.rs:81)
        out, p, produced = [], 0, 0
        while produced < length:
            if p + 4 + W > len(body):
                raise Malformed(E_IO, "rle runs")
            cnt = int.from_bytes(body[p:p + 4], "little")
            if produced + cnt > length:
                raise Malformed(E_OUT_OF_SPEC, "rle run overshoots")
            out.append(body[p + 4:p + 4 + W] * cnt)
            p += 4 + W
            produced += cnt
        out = b"".join(out)
    elif codec == ONE_VALUE:  # one_value.rs:77-94
        if len(body) < W:
            raise Malformed(E_IO, "one value")
        out = body[:W] * length
    elif codec == DICT:  # dict.rs:75-103
        idx, p = _oracle_call(O.decompress, body, np.uint32, length, 0)
        if p + 4 > len(body):
            raise Malformed(E_IO, "dict size")
        k = int.from_bytes(body[p:p + 4], "little")
        p += 4
        if k * W > len(body) - p:
            raise Malformed(E_OUT_OF_SPEC, "dict entries")
        if length and int(idx.max(initial=0)) >= k:
            raise Malformed(E_OUT_OF_SPEC, "dict index")
        out = b"".join(body[p + int(i) * W:p + int(i) * W + W] for i in idx)
    elif codec == FREQ:  # freq.rs:88-123
        if len(body) < W + 4:
            raise Malformed(E_IO, "freq top")
        bm = int.from_bytes(body[W:W + 4], "little")
        p = W + 4
        if p + bm > len(body):
            raise Malformed(E_IO, "freq bitmap")
        rows = _oracle_call(O.roaring_decode, body[p:p + bm])
        exc, _ = decompress_stream(body, p + bm, W, len(rows))
        cells = [body[:W]] * length
        for i, r in enumerate(rows):
            if int(r) >= length:
                raise Malformed(E_OUT_OF_SPEC, "freq row")
            cells[int(r)] = exc[i * W:(i + 1) * W]
        out = b"".join(cells)
    else:  # Bitpacking / DeltaBitpacking / Patas over 8-, 16- or 32-byte values, unknown codecs
        raise Malformed(E_OUT_OF_SPEC, f"codec {codec}")
    return out, pos + csize


def read_page(pg: bytes, n: int, W: int, nullable=False):
    """IntegerIter::deserialize on one page -> (n * W raw bytes, validity | None)."""
    pos, valid = 0, None
    if nullable:
        valid, pos = _oracle_call(O.read_validity, pg, n, 0)
    raw, _ = decompress_stream(pg, pos, W, n)
    return raw, valid


def read_column(chunk: bytes, metas, W: int, nullable=False):
    """-> (raw bytes of every row, validity | None); metas = [(length, num_values)]."""
    raws, valids, pos = [], [], 0
    for length, nv in metas:
        raw, v = read_page(chunk[pos:pos + length], nv, W, nullable)
        raws.append(raw)
        if nullable:
            valids.append(v)
        pos += length
    return b"".join(raws), (np.concatenate(valids) if nullable and valids else None)
