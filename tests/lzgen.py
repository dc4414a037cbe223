"""Hand-built LZ4 and Snappy streams for the decoder tests: token streams
written sequence by sequence (no compressor chooses them), plain Python
decoders that state from the format documents which streams are valid, seeded
case sets of sequence lists aimed at the device decoders' structural
boundaries, and wrappers that put a stream where the device routes it
differently.

The models restate the formats, not the device code:

* lz4_model: the LZ4 block format as LZ4_decompress_safe (liblz4 1.9, the
  reference's compression/basic.rs:87-91) accepts it with the exact output
  size.  The end-of-block rules of the format (lz4_Block_format.md, "End of
  block restrictions") are what the library checks: a non-final sequence's
  literals end at least 12 bytes before the end of the output and are followed
  by at least 8 input bytes, a match ends at least 5 bytes before the end of
  the output, and the last sequence is literals only and reaches both ends.
  One exception is the library's, not the format's: its "two-stage shortcut"
  copies a sequence with a literal length below 15, a match length below 19
  and an offset of 8 or more without the end checks when the sequence starts
  at least 32 bytes before the end of the output and more than 16 input bytes
  follow its token, so such a last match may run into the last 5 output bytes
  (and be followed by a tail shorter than 5).  The model states that exception
  as a separate clause, `_SHORTCUT`; tests/test_lz_model_cpu.py holds the
  model to liblz4 on every stream of classes A and B.
  One kind of stream is left out of those classes by construction: a match
  offset of 0.  The format forbids it and the model rejects it, but liblz4
  1.9 does not look: it copies from the match's own destination, so what it
  returns depends on what the output buffer held before.  No decoder can
  agree with that, so class B's edits set no offset to 0, the bit flips are
  drawn again when a zero offset is the first rule the flipped stream
  breaks, and lz4_offset0_cases() keeps the zero-offset edits apart: the
  model and the device must reject them, liblz4 is not asked.
* snappy_model: the Snappy raw format (format_description.txt) as Google's
  decoder accepts it.  Nothing here can build the reference's `snap` crate:
  Snappy reject parity is pinned to the oracle's decoder and to Google's
  (through pyarrow, where it imports), not to `snap`.  Those two differ on
  one stream kind, which the generators therefore never write: a literal
  whose 4-byte length field holds 0xFFFFFFFF (a length of 2^32).  Google's
  decoder adds the 1 in 32 bits and takes an empty literal; the oracle's,
  like this model, takes 2^32 bytes and rejects.

The page wrappers' `u32 usize` header field is read by neither the reference
(the oracle ignores it as compression/integer/mod.rs does) nor the device: the
decoders take the output size from the page's row count."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O

# the device decoder's geometry, as pa_amd/csrc/sb_decode.hip states it: the
# case sets aim at these boundaries, the models know nothing of them
RING, CHUNK = 2048, 512
DEFERRED_LDS, STAGE_PAD = 155 * 1024, 64


# --------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------
def _ext(n: int) -> bytes:
    """LZ4 length-extension bytes for the n beyond a nibble of 15."""
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_block(seqs, tail: bytes) -> bytes:
    """seqs: [(literal bytes, offset, match_len >= 4)], then the final
    literals-only sequence `tail`.  Any offset in 0..65535 is written as given."""
    out = bytearray()
    for lit, off, ml in seqs:
        assert ml >= 4 and 0 <= off <= 0xFFFF
        ln, m = len(lit), ml - 4
        out.append((min(ln, 15) << 4) | min(m, 15))
        if ln >= 15:
            out += _ext(ln - 15)
        out += lit
        out += off.to_bytes(2, "little")
        if m >= 15:
            out += _ext(m - 15)
    ln = len(tail)
    out.append(min(ln, 15) << 4)
    if ln >= 15:
        out += _ext(ln - 15)
    out += tail
    return bytes(out)


def lz4_replay(seqs, tail: bytes) -> bytes:
    out = bytearray()
    for lit, off, ml in seqs:
        out += lit
        _copy(out, off, ml)
    return bytes(out + tail)


def _copy(out: bytearray, off: int, n: int):
    assert 1 <= off <= len(out)
    if off >= n:
        s = len(out) - off
        out += out[s:s + n]
    else:
        pat = bytes(out[-off:])
        out += (pat * (n // off + 1))[:n]


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def snappy_block(elements, ulen=None) -> bytes:
    """elements: ("lit", bytes, nbytes in 0..4: the length encoding),
    ("copy1", off < 2048, len 4..11), ("copy2", off < 65536, len 1..64),
    ("copy4", off < 2^32, len 1..64); ulen: the preamble (default: the
    elements' output length)."""
    body = bytearray()
    total = 0
    for e in elements:
        kind = e[0]
        if kind == "lit":
            _, data, nb = e
            n = len(data) - 1
            assert n >= 0
            if nb == 0:
                assert n < 60
                body.append(n << 2)
            else:
                assert 1 <= nb <= 4 and n < 1 << (8 * nb)
                body.append((59 + nb) << 2)
                body += n.to_bytes(nb, "little")
            body += data
            total += len(data)
            continue
        _, off, ln = e
        if kind == "copy1":
            assert 4 <= ln <= 11 and 0 <= off < 2048
            body.append(1 | ((ln - 4) << 2) | ((off >> 8) << 5))
            body.append(off & 0xFF)
        elif kind == "copy2":
            assert 1 <= ln <= 64 and 0 <= off < 1 << 16
            body.append(2 | ((ln - 1) << 2))
            body += off.to_bytes(2, "little")
        else:
            assert kind == "copy4" and 1 <= ln <= 64 and 0 <= off < 1 << 32
            body.append(3 | ((ln - 1) << 2))
            body += off.to_bytes(4, "little")
        total += ln
    return varint(total if ulen is None else ulen) + bytes(body)


def snappy_replay(elements) -> bytes:
    out = bytearray()
    for e in elements:
        if e[0] == "lit":
            out += e[1]
        else:
            _copy(out, e[1], e[2])
    return bytes(out)


# --------------------------------------------------------------------------
# models
# --------------------------------------------------------------------------
_SHORTCUT = True  # liblz4's unchecked short-sequence path (module docstring)


def lz4_model(block: bytes, olen: int):
    """The bytes LZ4_decompress_safe writes for `block` when it returns
    exactly olen, else None."""
    return _lz4_walk(block, olen)[0]


def lz4_zero_offset(block: bytes, olen: int) -> bool:
    """The first rule `block` breaks is a match offset of 0."""
    return _lz4_walk(block, olen)[1]


def _lz4_walk(block: bytes, olen: int):
    return _lz4_walk_(block, olen) or (None, False)


def _lz4_walk_(block: bytes, olen: int):
    n = len(block)
    if n == 0:
        return None
    if olen == 0:  # the library's own special case: one token 0
        return (b"", False) if block == b"\x00" else None
    out = bytearray()
    ip = 0
    while True:
        if ip >= n:
            return None
        token = block[ip]
        ip += 1
        lit = token >> 4
        short = _SHORTCUT and lit != 15 and ip < n - 16 and len(out) <= olen - 32
        if lit == 15:
            while True:
                if ip >= n:
                    return None
                b = block[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        lit_in, lit_out = ip + lit, len(out) + lit
        if not short and (lit_out > olen - 12 or lit_in > n - 8):
            # only the last sequence may end here: literals to both ends
            if lit_in != n or lit_out != olen:
                return None
            out += block[ip:lit_in]
            return bytes(out), False
        out += block[ip:lit_in]
        ip = lit_in
        if ip + 2 > n:
            return None
        off = block[ip] | (block[ip + 1] << 8)
        ip += 2
        ml = token & 15
        unchecked = short and ml != 15 and off >= 8
        if ml == 15:
            while True:
                if ip >= n:
                    return None
                b = block[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if off == 0:
            return None, True
        if off > len(out):
            return None
        if not unchecked and len(out) + ml > olen - 5:
            return None
        _copy(out, off, ml)


def snappy_preamble(block: bytes):
    """(uncompressed length, its size in bytes): a varint of at most 32 bits, else None."""
    ulen = 0
    for k in range(min(5, len(block))):
        c = block[k]
        if k == 4 and (c & 0x7F) > 15:
            return None
        ulen |= (c & 0x7F) << (7 * k)
        if c < 0x80:
            return ulen, k + 1
    return None


def snappy_model(block: bytes, olen: int):
    """The bytes of a raw Snappy stream whose preamble and elements give
    exactly olen bytes, else None."""
    n = len(block)
    pre = snappy_preamble(block)
    if pre is None or pre[0] != olen:
        return None
    ip = pre[1]
    out = bytearray()
    while ip < n:
        tag = block[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if ip + nb > n:
                    return None
                ln = int.from_bytes(block[ip:ip + nb], "little")
                ip += nb
            ln += 1
            if ip + ln > n or len(out) + ln > olen:
                return None
            out += block[ip:ip + ln]
            ip += ln
            continue
        if kind == 1:
            if ip + 1 > n:
                return None
            ln = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | block[ip]
            ip += 1
        else:
            w = 2 if kind == 2 else 4
            if ip + w > n:
                return None
            ln = 1 + (tag >> 2)
            off = int.from_bytes(block[ip:ip + w], "little")
            ip += w
        if off == 0 or off > len(out) or len(out) + ln > olen:
            return None
        _copy(out, off, ln)
    return bytes(out) if len(out) == olen else None


def snappy_census(block: bytes) -> dict:
    """Element kinds of a valid stream: copy1 / copy2 / copy4 and lit0..lit4
    (the literal-length encodings)."""
    seen = {}
    ip = 0
    while block[ip] & 0x80:
        ip += 1
    ip += 1
    n = len(block)
    while ip < n:
        tag = block[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            nb = max(0, ln - 59)
            if nb:
                ln = int.from_bytes(block[ip:ip + nb], "little")
            ip += nb + ln + 1
            key = f"lit{nb}"
        else:
            ip += (1, 2, 4)[kind - 1]
            key = ("copy1", "copy2", "copy4")[kind - 1]
        seen[key] = seen.get(key, 0) + 1
    return seen


# --------------------------------------------------------------------------
# composing streams: literals and copies by output position
# --------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    codec: int        # O.LZ4 | O.SNAPPY
    block: bytes
    olen: int         # the output size the decoder is given
    out: object       # the plain replay (bytes), None for a stream built to be rejected
    seqs: object = None  # LZ4: (seqs, tail); Snappy: elements
    tags: tuple = field(default_factory=tuple)


class Comp:
    """A stream under construction: lit(n) appends n seeded literal bytes,
    copy(off, n) a match; `op` is the output position so far.  word=True
    keeps every aligned output word a small u32 (a Dict index below 4096):
    literal bytes by position, offsets rounded to a multiple of 4."""

    def __init__(self, rng, word=False, ascii=False):
        self.rng, self.word, self.ascii = rng, word, ascii
        self.ops = []  # ["lit", bytes, nbytes|None] | ["copy", off, n, kind|None]
        self.out = bytearray()

    @property
    def op(self):
        return len(self.out)

    def lit(self, n, nb=None):
        if n <= 0:
            return self
        b = self.rng.integers(0, 128 if self.ascii else 256, n, dtype=np.uint8)
        if self.word:
            q = (np.arange(n) + self.op) & 3
            b = np.where(q == 0, b, np.where(q == 1, b & 15, 0)).astype(np.uint8)
        return self.raw(b.tobytes(), nb)

    def raw(self, data: bytes, nb=None):
        """The given bytes as literals."""
        if not data:
            return self
        if self.ops and self.ops[-1][0] == "lit" and nb is None and self.ops[-1][2] is None:
            self.ops[-1][1] += data
        else:
            self.ops.append(["lit", data, nb])
        self.out += data
        return self

    def copy(self, off, n, kind=None):
        if self.word:
            off = max(4, off & ~3)
            if off > self.op:
                return self.lit(n)
        assert 1 <= off <= self.op and n >= 1, (off, self.op, n)
        self.ops.append(["copy", off, n, kind])
        _copy(self.out, off, n)
        return self

    # ---- LZ4
    def lz4(self, name, tags=()):
        """Close with a legal ending (a tail of at least 5 bytes, the last
        match starting at least 12 bytes before the end) and emit."""
        last = next((o for o in reversed(self.ops) if o[0] == "copy"), None)
        tail = len(self.ops[-1][1]) if self.ops and self.ops[-1][0] == "lit" else 0
        need = 5 if last is None else max(5, 12 - last[2])
        if last is None and not self.ops:
            need = 1
        if last is not None and tail < need:
            self.lit(need - tail)
        if self.word and self.op & 3:
            self.lit(4 - (self.op & 3))
        seqs, tail = self.lz4_seqs()
        block = lz4_block(seqs, tail)
        return Case(name, O.LZ4, block, self.op, bytes(self.out), (seqs, tail), tuple(tags))

    def lz4_seqs(self):
        seqs, pend = [], b""
        for o in self.ops:
            if o[0] == "lit":
                pend += o[1]
            else:
                assert o[2] >= 4
                seqs.append((pend, o[1], o[2]))
                pend = b""
        return seqs, pend

    # ---- Snappy
    def snappy(self, name, tags=(), prefer=("copy1", "copy2")):
        """Emit as Snappy: literals with their forced (or the shortest)
        length encoding, copies split into pieces of at most 64 bytes of the
        forced kind, else of the first kind in `prefer` that can hold them."""
        if self.word and self.op & 3:
            self.lit(4 - (self.op & 3))
        el = []
        for o in self.ops:
            if o[0] == "lit":
                data, nb = o[1], o[2]
                if nb is None:
                    n = len(data) - 1
                    nb = 0 if n < 60 else (n.bit_length() + 7) // 8
                el.append(("lit", data, nb))
                continue
            _, off, n, kind = o
            while n:
                k = kind
                m = min(n, 64)
                if k is None:
                    for k in prefer:
                        if k == "copy1" and off < 2048 and m >= 4:
                            m = min(m, 11)
                            break
                        if k == "copy2" and off < 1 << 16:
                            break
                        if k == "copy4":
                            break
                    else:
                        k = "copy2" if off < 1 << 16 else "copy4"
                elif k == "copy1":
                    m = min(m, 11)
                el.append((k, off, m))
                n -= m
        block = snappy_block(el)
        assert snappy_replay(el) == bytes(self.out)
        return Case(name, O.SNAPPY, block, self.op, bytes(self.out), el, tuple(tags))


def far_limit(op: int) -> int:
    """Below this output position the device reads history from HBM."""
    k = op // CHUNK
    return (k - 2) * CHUNK if k >= 2 else 0


LIT_LENS = [0, 1, 14, 15, 16, 63, 64, 65, 269, 270, 271, 2559, 2560, 2561]
MATCH_LENS = [4, 5, 18, 19, 20, 23, 24, 25, 63, 64, 65, 273, 274, 275, 511, 512, 513, 529, 2048, 5000]
OFFSETS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537,
           2047, 2048, 2049, 4096]


def _far_edges(c: Comp, ml: int, sep: int = 3):
    """Four matches of ml bytes whose sources end exactly at the device's
    far limit, start exactly at it, and straddle it by 1 and by ml - 1."""
    for which in range(4):
        f = far_limit(c.op)
        assert f >= ml, (c.op, f, ml)
        s = (f - ml, f, f - 1, f - ml + 1)[which]
        c.copy(c.op - s, ml)
        c.lit(sep)


def _shared_cases(rng, emit, minlen):
    """The sequence lists both codecs run (offset sets, far-limit edges);
    minlen: the codec's shortest copy."""
    cases = []
    # offsets, each with a free-path length (<= 24) and a hazard-path one, a few per stream
    for g in range(0, len(OFFSETS), 4):
        grp = OFFSETS[g:g + 4]
        c = Comp(rng).lit(max(grp) + int(rng.integers(1, 40)))
        for off in grp:
            for ml in (max(minlen, 7), 40):
                c.copy(off, ml).lit(int(rng.integers(0, 4)))
        cases.append(emit(c, f"offsets{grp[0]}-{grp[-1]}"))
    for ml in (8, 24, 25, 70):  # ml - 1, ml, ml + 1
        c = Comp(rng).lit(100)
        for off in (ml - 1, ml, ml + 1):
            c.copy(off, ml).lit(2)
        cases.append(emit(c, f"off_near_ml{ml}"))
    for n0 in (1, 5, 300, 1100, 3000):  # offset == op: the match reaches stream byte 0
        c = Comp(rng).lit(n0).copy(n0, max(minlen, 6)).lit(3)
        c.copy(c.op, 30).lit(1).copy(c.op, 9)
        cases.append(emit(c, f"off_is_op{n0}"))
    # far-limit edges at several positions inside a chunk, free and hazard lengths
    for r in (0, 1, 77, 300, 470, 511):
        for ml in (max(minlen, 4), 16, 24, 25, 40, 100):
            c = Comp(rng).lit(4 * CHUNK + r - 5).copy(17, 5)
            _far_edges(c, ml)
            cases.append(emit(c, f"far_r{r}_ml{ml}"))
    # the same with the matches packed back to back (one batch)
    for ml in (8, 24, 30):
        c = Comp(rng).lit(6 * CHUNK + 9)
        _far_edges(c, ml, sep=0)
        _far_edges(c, ml, sep=1)
        cases.append(emit(c, f"far_packed_ml{ml}"))
    return cases


@functools.lru_cache(maxsize=None)
def lz4_valid_cases():
    """Class A: valid LZ4 blocks, by sequence list."""
    rng = np.random.default_rng(0x124)
    cases = []

    def emit(c, name, tags=()):
        return c.lz4(name, tags)

    # literal lengths
    for n in LIT_LENS:
        c = Comp(rng).lit(20).copy(3, 6).lit(n).copy(19, 9)
        cases.append(emit(c, f"lit{n}"))
        c = Comp(rng).lit(n + 1).copy(1, 4).lit(n).copy(n + 5, 12)  # the first literal, and one later
        cases.append(emit(c, f"lit_first{n}"))
    # long literals (straight to HBM) starting at op % 512 in {0, 1, 511}
    for r in (0, 1, 511):
        for n in (2561, 3100, 4200):
            c = Comp(rng).lit(CHUNK + r - 8).copy(5, 8)
            assert c.op % CHUNK == r
            c.lit(n)
            c.copy(c.op - 3, 40).lit(2).copy(n // 2, 20).lit(1).copy(CHUNK + 7, 300)
            cases.append(emit(c, f"lit_global_r{r}_{n}"))
    # match lengths: overlapping, and from a source as long as the match where the size allows
    for ml in MATCH_LENS:
        if ml < 2048:
            c = Comp(rng).lit(100).copy(37, ml).lit(3).copy(int(rng.integers(1, 9)), ml)
            cases.append(emit(c, f"ml{ml}_overlap"))
        else:
            cases.append(emit(Comp(rng).lit(100).copy(37, ml), f"ml{ml}_overlap37"))
            cases.append(emit(Comp(rng).lit(100).copy(int(rng.integers(1, 9)), ml), f"ml{ml}_overlap"))
        if ml <= 2048:
            c = Comp(rng).lit(ml + 11).copy(ml + 7, ml).lit(1).copy(ml, ml)
            cases.append(emit(c, f"ml{ml}_disjoint"))
    cases += _shared_cases(rng, emit, 4)
    # offset 65535 (64 KiB + 256 of output)
    c = Comp(rng).lit(65536).copy(65535, 100).lit(5).copy(65535, 19).copy(65535, 4).lit(60)
    c.copy(65535, 40)
    assert c.op <= 65536 + 256
    c.lit(65536 + 256 - c.op)
    cases.append(emit(c, "off65535", ("big",)))
    # batch shapes
    c = Comp(rng).lit(16)
    for _ in range(200):  # 200 three-byte sequences: full 64-sequence batches
        c.copy(int(rng.integers(1, 17)), 4)
    cases.append(emit(c, "batch_200x3"))
    for j in range(0, 8):  # a successor on window positions 249..256 of a batch
        c = Comp(rng).lit(30).copy(9, 4).lit(j).copy(5, 4)
        for _ in range(120):
            c.copy(int(rng.integers(4, 30)), 4)
        cases.append(emit(c, f"batch_window_shift{j}"))
    for j in range(0, 6):  # the same with an extension byte in the sequence that crosses
        c = Comp(rng).lit(30).copy(9, 4).lit(j).copy(5, 4)
        for _ in range(82):
            c.copy(int(rng.integers(4, 30)), 4)
        c.lit(15 + j).copy(11, 19 + j)
        for _ in range(20):
            c.copy(int(rng.integers(4, 30)), 5)
        cases.append(emit(c, f"batch_window_ext{j}"))
    for total in (511, 512, 513):  # a batch's output: one chunk at most
        c = Comp(rng).lit(65).copy(33, 31)  # (the long literal goes the serial way: the batch starts after it)
        for _ in range(31):
            c.copy(16, 16)
        c.copy(16, total - 31 * 16)
        for _ in range(10):
            c.copy(8, 8)
        cases.append(emit(c, f"batch_out{total}"))
    for lit in (0, 2):  # chains: each match copies the previous match's output inside a batch
        c = Comp(rng).lit(40)
        for _ in range(50):
            c.lit(lit).copy(8 + lit, 8)
        cases.append(emit(c, f"batch_chain_lit{lit}"))
    c = Comp(rng).lit(40)
    for i in range(60):  # self-overlap inside a batch
        c.lit(i % 3).copy(1 + i % 7, 9 + i % 22)
    cases.append(emit(c, "batch_self_overlap"))
    # input ring: 1.5 - 3 KiB of dense short sequences, every alignment of token,
    # extension byte and offset against the 512-byte input boundaries
    for j in range(9):
        c = Comp(rng).lit(40 + j)
        k = 0
        while True:
            seqs, tail = c.lz4_seqs()
            if len(lz4_block(seqs, tail)) > 1536 + 170 * j:
                break
            k += 1
            c.lit((0, 1, 15, 16, 0, 2)[k % 6]).copy(int(rng.integers(1, 40)), (4, 19, 20, 5, 34)[k % 5])
        cases.append(emit(c, f"input_ring_shift{j}"))
    # legal endings
    for tail in range(5, 21):
        c = Comp(rng).lit(30).copy(7, 11).lit(2).copy(20, 9).lit(tail)
        cases.append(emit(c, f"tail{tail}"))
    c = Comp(rng).lit(30).copy(7, 11).lit(2).copy(20, 4).lit(8)  # the last match starts 12 before the end
    cases.append(emit(c, "last_match_at_12"))
    c = Comp(rng).lit(30).copy(7, 11).lit(5)  # the last match ends 5 before the end
    cases.append(emit(c, "last_match_ends_at_5"))
    for n in (1, 4, 5, 12, 15, 64, 600, 3000):  # literals only
        cases.append(emit(Comp(rng).lit(n), f"literal_only{n}"))
    # random mixes of the value sets
    for t in range(40):
        c = Comp(rng).lit(int(rng.integers(1, 80)))
        while c.op < int(rng.integers(600, 7000)):
            c.lit(int(rng.choice(LIT_LENS[:11])) if rng.random() < 0.7 else 0)
            off = int(rng.choice(OFFSETS))
            ml = int(rng.choice(MATCH_LENS[:17]))
            if rng.random() < 0.3 and far_limit(c.op) >= ml:
                off = c.op - (far_limit(c.op) - int(rng.integers(0, ml + 1)))
            c.copy(min(off, c.op), ml)
        cases.append(emit(c, f"mix{t}"))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def snappy_valid_cases():
    """Class A: valid Snappy streams, by element list."""
    rng = np.random.default_rng(0x5A)
    cases = []

    def emit(c, name, tags=()):
        return c.snappy(name, tags, prefer=("copy2",))

    # every literal-length encoding (tags 60..63 with 1..4 length bytes), short and long literals
    for nb in range(5):
        for n in {0: (1, 59, 60), 1: (1, 61, 256), 2: (7, 257, 3000), 3: (3, 70, 2600), 4: (9, 300, 2561)}[nb]:
            c = Comp(rng).lit(33).copy(7, 5).lit(n, nb=nb).copy(n + 3, 11).lit(2, nb=nb)
            cases.append(c.snappy(f"lit_nb{nb}_{n}"))
    # copy-2 of length 1, 2, 3 (copy-1 cannot be that short), every copy length 1..64
    c = Comp(rng).lit(50)
    for ln in range(1, 65):
        c.copy(int(rng.integers(1, 50)), ln, "copy2").lit(ln % 3)
    cases.append(c.snappy("copy2_len1-64"))
    c = Comp(rng).lit(50)
    for ln in range(1, 65):
        c.copy(int(rng.integers(1, 50)), ln, "copy4").lit(ln % 2)
    cases.append(c.snappy("copy4_len1-64"))
    # copy-1: every length, the offsets at its edges
    for off in (1, 63, 64, 65, 255, 256, 2047):
        c = Comp(rng).lit(off + 5)
        for ln in range(4, 12):
            c.copy(off, ln, "copy1").lit(ln % 3)
        cases.append(c.snappy(f"copy1_off{off}"))
    # copy-4 past 65535, and small offsets it may also carry
    c = Comp(rng).lit(65600).copy(65536, 64, "copy4").copy(65536, 33, "copy4").lit(3)
    c.copy(65537, 1, "copy4").copy(5, 20, "copy4").copy(c.op, 7, "copy4")
    c.lit(69999 - c.op).copy(69999, 1, "copy4")
    assert c.op == 70000
    cases.append(c.snappy("copy4_far", ("big",)))
    # preamble varints of 1, 2 and 3 bytes
    for n in (1, 127, 128, 16383, 16384):
        c = Comp(rng).lit(min(n, 40))
        while c.op < n:
            m = min(n - c.op, int(rng.integers(1, 65)))
            c.copy(int(rng.integers(1, min(c.op, 60) + 1)), m) if rng.random() < 0.8 else c.lit(m)
        assert c.op == n
        cases.append(c.snappy(f"varint_{n}", ("big",) if n > 8192 else ()))
    cases += _shared_cases(rng, emit, 1)
    # the same sequence lists with copy-1 wherever it fits
    cases += [Case(k.name + "_c1", *_reencode(k)) for k in _shared_cases(np.random.default_rng(0x5B), emit, 4)[:12]]
    # dense short elements (compressed 1.5 - 3 KiB)
    for j in range(4):
        c = Comp(rng).lit(40 + j)
        for k in range(520 + 120 * j):
            c.lit((0, 1, 0, 2)[k % 4]).copy(int(rng.integers(1, 40)), (4, 1, 11, 5, 2)[k % 5])
        cases.append(c.snappy(f"dense{j}"))
    # random mixes
    for t in range(30):
        c = Comp(rng).lit(int(rng.integers(1, 80)))
        while c.op < int(rng.integers(600, 7000)):
            c.lit(int(rng.choice(LIT_LENS[:11])) if rng.random() < 0.7 else 0,
                  nb=int(rng.integers(3, 5)) if rng.random() < 0.1 else None)
            off = int(rng.choice(OFFSETS))
            ml = int(rng.choice([1, 2, 3] + MATCH_LENS[:14]))
            if rng.random() < 0.3 and far_limit(c.op) >= ml:
                off = c.op - (far_limit(c.op) - int(rng.integers(0, ml + 1)))
            c.copy(min(off, c.op), ml, "copy4" if rng.random() < 0.1 else None)
        cases.append(c.snappy(f"mix{t}", prefer=("copy1", "copy2") if t % 2 else ("copy2",)))
    return tuple(cases)


def _reencode(k: Case):
    """A Snappy case's elements with copy-1 in place of every copy-2 it can replace."""
    el = []
    for e in k.seqs:
        if e[0] == "copy2" and e[1] < 2048 and e[2] >= 4:
            n = e[2]
            while n:
                m = min(n, 11) if n - min(n, 11) == 0 or n - min(n, 11) >= 4 else n - 4
                el.append(("copy1", e[1], m) if 4 <= m <= 11 else ("copy2", e[1], m))
                n -= m
        else:
            el.append(e)
    assert snappy_replay(el) == k.out
    return k.codec, snappy_block(el), k.olen, k.out, el, k.tags


@functools.lru_cache(maxsize=None)
def word_cases(codec: int):
    """Valid streams whose every aligned output word is a u32 below 4096, for
    the placements that read the output as Dict indices: the random mixes and
    batch shapes with offsets that are multiples of 4."""
    rng = np.random.default_rng(0xD1C7 + codec)
    cases = []
    for t in range(24):
        c = Comp(rng, word=True).lit(int(rng.integers(4, 80)))
        while c.op < int(rng.integers(600, 7000)):
            c.lit(int(rng.choice(LIT_LENS[:11])) if rng.random() < 0.7 else 0)
            off = int(rng.choice(OFFSETS)) + int(rng.integers(0, 4))
            ml = int(rng.choice(MATCH_LENS[:17]))
            if rng.random() < 0.3 and far_limit(c.op) >= ml:
                off = c.op - (far_limit(c.op) - int(rng.integers(0, ml + 1)))
            c.copy(min(off, c.op), ml)
        cases.append(c.lz4(f"wmix{t}") if codec == O.LZ4 else c.snappy(f"wmix{t}"))
    for j in range(4):
        c = Comp(rng, word=True).lit(40 + j)
        for k in range(300):
            c.lit((0, 1, 0, 15)[k % 4]).copy(4 * int(rng.integers(1, 12)), (4, 8, 11, 5, 19)[k % 5])
        cases.append(c.lz4(f"wdense{j}") if codec == O.LZ4 else c.snappy(f"wdense{j}"))
    return tuple(cases)


# --------------------------------------------------------------------------
# class B: streams edited to break one rule each, and seeded bit flips
# --------------------------------------------------------------------------
def _bases(cases, count, max_olen=3000):
    small = [k for k in cases if k.olen <= max_olen and "big" not in k.tags]
    step = max(1, len(small) // count)
    return small[::step][:count]


@functools.lru_cache(maxsize=None)
def lz4_edit_cases():
    """Class B for LZ4: each base stream with one rule of the block format
    broken.  `out` is None: the expected verdict is the model's."""
    rng = np.random.default_rng(0xB4)
    out = []

    def add(name, block, olen):
        out.append(Case(name, O.LZ4, bytes(block), olen, None))

    # blocks that obey every rule but the end-of-block ones
    lit12 = bytes(range(12))
    add("end:tail4", lz4_block([(lit12 * 2, 5, 20)], b"abcd"), 48)
    add("end:tail0", lz4_block([(lit12 * 2, 5, 20)], b""), 44)
    s71 = [(lit12, 3, 4)] + [(b"", 4, 4)] * 70
    add("end:71_matches_tail5", lz4_block(s71, b"abcde"), 12 + 71 * 4 + 5)
    add("end:lit12_match4_tail5", lz4_block([(lit12, 7, 4)], b"abcde"), 21)
    for k in _bases([c for c in lz4_valid_cases() if c.seqs[0]], 36):
        seqs, tail = k.seqs
        body = lz4_replay(seqs, b"")
        for t in range(0, 5):  # tails of 0..4 bytes: the last match ends within the last 5 bytes
            add(f"{k.name}:tail{t}", lz4_block(seqs, tail[:t]), len(body) + t)
        # the last non-final sequence's literals end within the last 12 output bytes
        # (a 4-byte match and a 5..7-byte tail behind them)
        lit, off, _ = seqs[-1]
        for t in (5, 6, 7):
            s2 = seqs[:-1] + [(lit, off, 4)]
            add(f"{k.name}:lit_end_{4 + t}", lz4_block(s2, tail[:5] + bytes(t - 5)), len(lz4_replay(s2, b"")) + t)
        # fewer than 8 input bytes behind a non-final sequence's literals: offset,
        # token and a tail shorter than 5, behind a match long enough to satisfy the output rules' other half
        s2 = seqs[:-1] + [(lit, off, 40)]
        add(f"{k.name}:input_7", lz4_block(s2, tail[:4]), len(lz4_replay(s2, b"")) + 4)
        # a match ending within the last 5 bytes behind a long literal (no short-sequence path)
        s2 = seqs[:-1] + [(lit + bytes(20), off, 30)]
        for t in (0, 3, 4):
            add(f"{k.name}:match_end_{t}", lz4_block(s2, tail[:t]), len(lz4_replay(s2, b"")) + t)
        # liblz4's unchecked short sequences (module docstring): a last match of
        # at most 18 bytes at an offset of 8 or more behind at most 14 literals
        # may end anywhere; one step outside each of those bounds may not
        pre = seqs[:-1] + [(lit + bytes(40), off, 8)]
        for nl, o2, ml, t in ((14, 8, 18, 0), (14, 9, 18, 4), (12, 30, 18, 4), (14, 8, 14, 4), (14, 8, 17, 1),
                              (14, 7, 18, 0), (14, 8, 19, 0), (15, 8, 18, 0), (11, 8, 18, 2), (14, 8, 13, 4)):
            s2 = pre + [(bytes(range(nl)), o2, ml)]
            add(f"{k.name}:short_l{nl}_o{o2}_m{ml}_t{t}", lz4_block(s2, tail[:t]), len(lz4_replay(s2, b"")) + t)
        # one past the start of the stream
        j = int(rng.integers(0, len(seqs)))
        s2 = list(seqs)
        opj = len(lz4_replay(seqs[:j], b"")) + len(seqs[j][0])
        if opj + 1 <= 0xFFFF:
            s2[j] = (seqs[j][0], opj + 1, seqs[j][2])
            add(f"{k.name}:off_op+1_seq{j}", lz4_block(s2, tail), k.olen)
        # truncated, a trailing byte, the output size off by one
        for cut in (1, 2, int(rng.integers(3, len(k.block))), len(k.block) // 2):
            add(f"{k.name}:cut{cut}", k.block[:-cut], k.olen)
        add(f"{k.name}:trail00", k.block + b"\x00", k.olen)
        add(f"{k.name}:trail50", k.block + b"\x50", k.olen)
        add(f"{k.name}:olen+1", k.block, k.olen + 1)
        add(f"{k.name}:olen-1", k.block, k.olen - 1)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lz4_offset0_cases():
    """Base streams with one match offset set to 0 (module docstring: the
    format forbids it, liblz4 does not look)."""
    rng = np.random.default_rng(0xB0)
    out = []
    for k in _bases([c for c in lz4_valid_cases() if c.seqs[0]], 36):
        seqs, tail = k.seqs
        j = int(rng.integers(0, len(seqs)))
        s2 = list(seqs)
        s2[j] = (seqs[j][0], 0, seqs[j][2])
        out.append(Case(f"{k.name}:off0_seq{j}", O.LZ4, lz4_block(s2, tail), k.olen, None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def snappy_edit_cases():
    rng = np.random.default_rng(0xB5)
    out = []

    def add(name, block, olen):
        out.append(Case(name, O.SNAPPY, bytes(block), olen, None))

    for k in _bases([c for c in snappy_valid_cases() if any(e[0] != "lit" for e in c.seqs)], 36):
        el = list(k.seqs)
        copies = [i for i, e in enumerate(el) if e[0] != "lit"]
        j = copies[int(rng.integers(0, len(copies)))]
        kind, off, ln = el[j]
        e2 = list(el)
        e2[j] = (kind, 0, ln)
        add(f"{k.name}:off0_el{j}", snappy_block(e2), k.olen)
        opj = len(snappy_replay(el[:j]))
        if opj + 1 < (2048 if kind == "copy1" else 1 << 16):
            e2[j] = (kind, opj + 1, ln)
            add(f"{k.name}:off_op+1_el{j}", snappy_block(e2), k.olen)
        for cut in (1, 2, int(rng.integers(3, len(k.block))), len(k.block) // 2):
            add(f"{k.name}:cut{cut}", k.block[:-cut], k.olen)
        add(f"{k.name}:trail00", k.block + b"\x00", k.olen)
        add(f"{k.name}:trail_copy", k.block + b"\x05", k.olen)
        add(f"{k.name}:olen+1", k.block, k.olen + 1)
        add(f"{k.name}:olen-1", k.block, k.olen - 1)
        add(f"{k.name}:ulen+1", snappy_block(el, ulen=k.olen + 1), k.olen)
        add(f"{k.name}:ulen-1", snappy_block(el, ulen=k.olen - 1), k.olen)
        add(f"{k.name}:ulen+1_both", snappy_block(el, ulen=k.olen + 1), k.olen + 1)
        add(f"{k.name}:one_more_copy", snappy_block(el + [("copy2", 1, 1)], ulen=k.olen), k.olen)
        # literal lengths past the input (not 2^32: module docstring)
        for nb, v in ((1, 0xFF), (2, 0xFFFF), (3, 0xFFFFFF), (4, 0xFFFFFFFE), (4, 0x7FFFFFFF)):
            add(f"{k.name}:lit_len_{nb}_{v:x}", k.block + bytes([(59 + nb) << 2]) + v.to_bytes(nb, "little"), k.olen)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flip_cases(codec: int, count: int = 300):
    """A fixed seeded set of 1-3 bit flips per stream (LZ4: drawn again when
    the flips make a zero offset the stream's first fault, module docstring)."""
    rng = np.random.default_rng(0xF11 + codec)
    bases = _bases(lz4_valid_cases() if codec == O.LZ4 else snappy_valid_cases(), 50, 2600)
    out = []
    for t in range(count):
        k = bases[t % len(bases)]
        while True:
            b = bytearray(k.block)
            for _ in range(int(rng.integers(1, 4))):
                i = int(rng.integers(0, len(b)))
                b[i] ^= 1 << int(rng.integers(0, 8))
            if codec != O.LZ4 or not lz4_zero_offset(bytes(b), k.olen):
                break
        out.append(Case(f"{k.name}:flip{t}", codec, bytes(b), k.olen, None))
    return tuple(out)


def model(k: Case):
    return (lz4_model if k.codec == O.LZ4 else snappy_model)(k.block, k.olen)


def oracle_verdict(k: Case):
    """The oracle's decoder (liblz4 / its Snappy decoder): bytes or None."""
    try:
        return O.common_decompress(k.codec, k.block, k.olen)
    except O.OracleError:
        return None


# --------------------------------------------------------------------------
# page wrappers
# --------------------------------------------------------------------------
def stream(codec: int, block: bytes, usize: int) -> bytes:
    """[codec][u32 csize][u32 usize][block]"""
    return bytes([codec]) + len(block).to_bytes(4, "little") + (usize & 0xFFFFFFFF).to_bytes(4, "little") + block


def validity_bits(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random(n) > 0.3


def leaf_page(k: Case, validity=None, usize=None) -> tuple:
    """P1: the stream as an Int8 page's values -> (page, rows)."""
    pre = O.write_validity(validity) if validity is not None else b""
    return pre + stream(k.codec, k.block, k.olen if usize is None else usize), k.olen


def freq_rows(olen: int) -> tuple:
    """Rows of a Freq page with olen exceptions: every fourth row holds the top value."""
    n = olen + olen // 3 + 1
    pos = np.flatnonzero(np.arange(n) % 4 != 3)[:olen]
    return n, pos.astype(np.uint32)


FREQ_TOP = 0x5C


def freq_page(k: Case, validity=None) -> tuple:
    """P2: the stream as the exceptions of an Int8 Freq page
    [13][csize][usize][top][u32 bitmap size][roaring][exceptions stream]
    (integer/freq.rs:88-123), small enough for the deferred pass's LDS."""
    n, pos = freq_rows(k.olen)
    roar = O.roaring_encode(pos)
    body = bytes([FREQ_TOP]) + len(roar).to_bytes(4, "little") + roar + stream(k.codec, k.block, k.olen)
    pre = O.write_validity(validity) if validity is not None else b""
    return pre + stream(O.FREQ, body, n), n


def freq_expected(k: Case, out: bytes) -> np.ndarray:
    n, pos = freq_rows(k.olen)
    v = np.full(n, FREQ_TOP, np.uint8)
    v[pos] = np.frombuffer(out, np.uint8)
    return v


DICT_K = 4096


def dict_values(k: int) -> np.ndarray:
    return ((np.arange(k, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)


def dict_page(k: Case, validity=None, entries: int = DICT_K) -> tuple:
    """P2 / P3: the stream as the u32 index stream of an Int8 Dict page
    [11][csize][usize][index stream][u32 k][k values] (integer/dict.rs:75-103);
    k.olen is a multiple of 4 and every index below DICT_K (word_cases)."""
    assert k.olen % 4 == 0
    n = k.olen // 4
    body = stream(k.codec, k.block, k.olen) + entries.to_bytes(4, "little") + dict_values(entries).tobytes()
    pre = O.write_validity(validity) if validity is not None else b""
    return pre + stream(O.DICT, body, n), n


def dict_expected(out: bytes) -> np.ndarray:
    return dict_values(DICT_K)[np.frombuffer(out, "<u4")]


def spill_entries(k: Case, validity=None) -> int:
    """P3: the fewest dictionary entries with which the page still fits the
    deferred pass's LDS but its expanded index stream no longer does
    (decode_page MODE 1: bytes > stage - align16(len + 15 + pad) - pad), so
    the stream is queued for expansion into HBM."""
    base = len(dict_page(k, validity, 0)[0])
    e = DEFERRED_LDS - 2 * STAGE_PAD - 31 - k.olen - base
    while True:
        need = (base + e + 15 + STAGE_PAD + 15) & ~15
        if k.olen > DEFERRED_LDS - need - STAGE_PAD:
            assert need + 64 <= DEFERRED_LDS
            return e
        e += 1


# --------------------------------------------------------------------------
# P4: Binary / Utf8 Basic pages (binary/mod.rs:95-183): both streams hand-built
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ascii_cases(codec: int):
    """Valid streams of ASCII bytes (a Utf8 page's values): random mixes."""
    rng = np.random.default_rng(0xA5C + codec)
    cases = []
    for t in range(16):
        c = Comp(rng, ascii=True).lit(int(rng.integers(1, 80)))
        while c.op < int(rng.integers(600, 7000)):
            c.lit(int(rng.choice(LIT_LENS[:11])) if rng.random() < 0.7 else 0)
            off = int(rng.choice(OFFSETS))
            ml = int(rng.choice(MATCH_LENS[:17]))
            if rng.random() < 0.3 and far_limit(c.op) >= ml:
                off = c.op - (far_limit(c.op) - int(rng.integers(0, ml + 1)))
            c.copy(min(off, c.op), ml)
        cases.append(c.lz4(f"amix{t}") if codec == O.LZ4 else c.snappy(f"amix{t}"))
    return tuple(cases)


def offsets_case(codec: int, ow: int, total: int, seed: int) -> Case:
    """A hand-built stream that decodes to the page-local offsets of a Basic
    page whose values hold `total` bytes: runs of equal offsets (rows of empty
    strings), a few of them longer than the device's history ring, so a match
    at any multiple of the offset width inside a run is valid -- near, far
    (read back from the column, where the offsets already lie rebased) and
    straddling the far limit -- at any length."""
    rng = np.random.default_rng(seed)
    runs = int(rng.integers(6, 14))
    vals = [0] + sorted(int(x) for x in rng.integers(0, total + 1, runs - 2)) + [total]
    c = Comp(rng)
    for r, v in enumerate(vals):
        word = v.to_bytes(ow, "little")
        start = c.op
        last = r == len(vals) - 1
        n = 4 if last else int(rng.integers(600, 1000)) if r % 4 == 1 else int(rng.integers(1, 7))
        c.raw(word)
        left = (n - 1) * ow
        while left:
            m = min(left, int(rng.choice(MATCH_LENS[:14])))
            if last or rng.random() < 0.2 or (codec == O.LZ4 and m < 4):  # a literal piece of the run
                m = min(left, int(rng.integers(1, 20))) if not last else left
                phase = (c.op - start) % ow
                c.raw((word * (m // ow + 2))[phase:phase + m])
            else:
                words = (c.op - start) // ow
                j = words if rng.random() < 0.3 else int(rng.integers(1, words + 1))
                c.copy(ow * j, m)
            left -= m
    assert c.op % ow == 0 and np.all(np.diff(np.frombuffer(bytes(c.out), f"<u{ow}").astype(np.int64)) >= 0)
    return c.lz4(f"offsets{seed}") if codec == O.LZ4 else c.snappy(f"offsets{seed}")


def binary_page(offs: Case, vals: Case, ow: int, validity=None) -> tuple:
    """[codec][csize][usize][offsets stream][codec][csize][usize][values stream] -> (page, rows)"""
    assert offs.codec == vals.codec
    pre = O.write_validity(validity) if validity is not None else b""
    return pre + stream(offs.codec, offs.block, offs.olen) + stream(vals.codec, vals.block, vals.olen), offs.olen // ow - 1


def binary_column(codec: int, ow: int, vals_cases, nullable: bool):
    """One column of P4 pages, one per values case -> (pages [(bytes, rows)],
    offsets of the whole column (int64), values bytes, validity | None)."""
    pages, offs, vals, valid = [], [np.zeros(1, np.int64)], [], []
    base = 0
    for i, v in enumerate(vals_cases):
        o = offsets_case(codec, ow, v.olen, 1000 * ow + 10 * i + codec)
        rows = o.olen // ow - 1
        val = validity_bits(rows, i) if nullable else None
        pages.append(binary_page(o, v, ow, val))
        local = np.frombuffer(o.out, f"<u{ow}").astype(np.int64)
        offs.append(base + local[1:])
        base += v.olen
        vals.append(v.out)
        if nullable:
            valid.append(val)
    return pages, np.concatenate(offs), b"".join(vals), np.concatenate(valid) if nullable else None
