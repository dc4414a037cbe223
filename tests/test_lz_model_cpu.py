"""The LZ4 and Snappy models of tests/lzgen.py against the libraries, on any
host: before a GPU test relies on a model's verdict, the model must give
liblz4's (LZ4_decompress_safe with the exact output size, through the oracle)
on every hand-built stream, every edited one and every bit-flipped one, with
no exceptions; the Snappy model must give the oracle decoder's and, where
pyarrow imports, Google's.  Snappy reject parity is pinned to those two
decoders: the reference's `snap` crate cannot be built here.  Zero-offset LZ4
matches are the one kind liblz4 is not asked about (tests/lzgen.py explains
why); the model rejects them as the format does."""
import collections

import numpy as np
import pytest

from oracle import oracle as O
from tests import lzgen as G


def _agree(cases):
    """Model and oracle verdicts over `cases`: no disagreement in verdict or
    bytes -> Counter of verdicts."""
    seen = collections.Counter()
    bad = []
    for k in cases:
        m, o = G.model(k), G.oracle_verdict(k)
        if m != o:
            bad.append(f"{k.name}: model {'rejects' if m is None else 'decodes'}, "
                       f"library {'rejects' if o is None else 'decodes'}")
        seen["err" if m is None else "ok"] += 1
    assert not bad, f"{len(bad)} of {len(cases)} disagree: {bad[:8]}"
    return seen


@pytest.mark.parametrize("codec", [O.LZ4, O.SNAPPY], ids=["lz4", "snappy"])
def test_valid_streams_replay(codec):
    """Class A: the builder's bytes decode, with the model and with the
    library, to the plain replay of the sequence list."""
    cases = (G.lz4_valid_cases() if codec == O.LZ4 else G.snappy_valid_cases()) + G.word_cases(codec)
    assert len(cases) > 100
    for k in cases:
        replay = G.lz4_replay(*k.seqs) if codec == O.LZ4 else G.snappy_replay(k.seqs)
        assert replay == k.out and len(replay) == k.olen, k.name
        assert G.model(k) == k.out, f"{k.name}: model"
        assert G.oracle_verdict(k) == k.out, f"{k.name}: library"


def test_case_sizes():
    """Outputs stay small: 8 KiB, but for the offset-65535 case, the copy-4
    case and the two cases at the edge of a 3-byte preamble (16 KiB)."""
    for k in G.lz4_valid_cases() + G.snappy_valid_cases():
        assert k.olen <= (70000 if "big" in k.tags else 8192), k.name
    assert sum("big" in k.tags for k in G.lz4_valid_cases() + G.snappy_valid_cases()) == 4
    # the input-ring cases: 1.5 - 3 KiB of compressed bytes
    ring = [len(k.block) for k in G.lz4_valid_cases() if k.name.startswith("input_ring")]
    assert len(ring) == 9 and min(ring) >= 1536 and max(ring) <= 3072


def test_lz4_edits_match_liblz4():
    seen = _agree(G.lz4_edit_cases())
    print("lz4 edits:", dict(seen))
    assert seen["ok"] and seen["err"]  # (the accepted ones: liblz4's unchecked short sequences)
    named = {k.name: k for k in G.lz4_edit_cases() if k.name.startswith("end:")}
    assert len(named) == 4 and all(G.model(k) is None for k in named.values())


def test_lz4_flips_match_liblz4():
    cases = G.flip_cases(O.LZ4)
    assert len(cases) == 300
    seen = _agree(cases)
    print("lz4 flips:", dict(seen))
    assert seen["ok"] and seen["err"]


def test_lz4_end_rules_one_by_one():
    """Every split of a short block into literals, one match and a tail,
    against liblz4: the end rules and the library's unchecked short sequences
    at each distance from the end."""
    cases = []
    for nl in (0, 1, 11, 12, 13, 14, 15, 16, 30):
        for ml in (4, 5, 7, 8, 17, 18, 19, 20, 40):
            for off in (1, 7, 8, 9):
                for tail in range(0, 14):
                    for pre in (0, 40):
                        seqs = ([(bytes(range(pre)), 3, 9)] if pre else []) + [(bytes(range(9, 9 + nl)), off, ml)]
                        if not pre and off > nl:
                            continue
                        olen = len(G.lz4_replay(seqs, b"")) + tail
                        cases.append(G.Case(f"l{nl}_m{ml}_o{off}_t{tail}_p{pre}", O.LZ4,
                                            G.lz4_block(seqs, bytes(tail)), olen, None))
    seen = _agree(cases)
    print("lz4 end rules:", dict(seen), "of", len(cases))
    assert seen["ok"] > 1000 and seen["err"] > 1000


def test_lz4_zero_offsets_rejected_by_model():
    cases = G.lz4_offset0_cases()
    assert len(cases) == 36
    for k in cases:
        assert G.model(k) is None and G.lz4_zero_offset(k.block, k.olen), k.name
    for k in G.lz4_edit_cases() + G.flip_cases(O.LZ4):
        assert not G.lz4_zero_offset(k.block, k.olen), k.name


def _google(k):
    """Google's decoder through pyarrow, asked only when the preamble names
    the size the caller expects (its API takes that size on trust)."""
    import pyarrow as pa

    try:
        return pa.Codec("snappy").decompress(k.block, decompressed_size=k.olen).to_pybytes()
    except (pa.ArrowException, OSError, ValueError):
        return None


def test_snappy_edits_and_flips_match_decoders():
    try:
        import pyarrow as pa

        google = pa.Codec.is_available("snappy")
    except ImportError:
        google = False
    cases = G.snappy_edit_cases() + G.flip_cases(O.SNAPPY)
    seen = _agree(cases)
    print("snappy edits and flips:", dict(seen), "pyarrow:", google)
    assert seen["ok"] and seen["err"]
    assert len(G.flip_cases(O.SNAPPY)) == 300
    if google:
        asked = 0
        for k in cases + G.snappy_valid_cases():
            pre = G.snappy_preamble(k.block)
            if pre is None or pre[0] != k.olen:
                assert G.model(k) is None, k.name
                continue
            asked += 1
            assert _google(k) == G.model(k), f"{k.name}: Google's decoder and the model differ"
        assert asked > 400


def test_snappy_tag_census():
    """Class A holds the element kinds no compressor-made stream of the suite
    has: copy-1, copy-4 and literal lengths of 3 and 4 bytes."""
    cen = collections.Counter()
    for k in G.snappy_valid_cases():
        cen.update(G.snappy_census(k.block))
    print("snappy elements:", dict(cen))
    for key in ("copy1", "copy2", "copy4", "lit0", "lit1", "lit2", "lit3", "lit4"):
        assert cen[key] >= 10, key


def test_lz4_census():
    """Class A reaches the lengths and offsets the device decoder branches on."""
    lits, mls, offs = set(), set(), set()
    for k in G.lz4_valid_cases():
        for lit, off, ml in k.seqs[0]:
            lits.add(len(lit))
            mls.add(ml)
            offs.add(off)
    assert set(G.LIT_LENS) <= lits and set(G.MATCH_LENS) <= mls and set(G.OFFSETS) | {65535} <= offs


def test_page_wrappers_decode_with_the_oracle():
    """The placements are pages the reference reads: the oracle decodes each
    wrapper to the stream's bytes (the header's usize off by one included)."""
    for codec in (O.LZ4, O.SNAPPY):
        cases = (G.lz4_valid_cases() if codec == O.LZ4 else G.snappy_valid_cases())[::9]
        for i, k in enumerate(cases):
            for nullable in (False, True):
                val = G.validity_bits(k.olen, i) if nullable else None
                page, n = G.leaf_page(k, val, usize=k.olen + i % 3 - 1)
                v, m = O.read_page(page, n, np.int8, nullable)
                assert v.tobytes() == k.out, k.name
                assert not nullable or (m == val).all()
                n2 = G.freq_rows(k.olen)[0]
                val = G.validity_bits(n2, i) if nullable else None
                page, n = G.freq_page(k, val)
                v, m = O.read_page(page, n, np.int8, nullable)
                assert v.view(np.uint8).tobytes() == G.freq_expected(k, k.out).tobytes(), k.name
                assert not nullable or (m == val).all()
        for i, k in enumerate(G.word_cases(codec)[::5]):
            for entries in (G.DICT_K, G.spill_entries(k)):
                page, n = G.dict_page(k, None, entries)
                v, _ = O.read_page(page, n, np.int8, False)
                assert v.view(np.uint8).tobytes() == G.dict_expected(k.out).tobytes(), k.name
            # the spill size: the page fits the deferred pass's LDS, page and index stream together do not
            need = (len(page) + 15 + G.STAGE_PAD + 15) & ~15
            assert need + 64 <= G.DEFERRED_LDS < need + G.STAGE_PAD + k.olen
            small, _ = G.dict_page(k, None, entries - 16)
            assert ((len(small) + 15 + G.STAGE_PAD + 15) & ~15) + G.STAGE_PAD + k.olen <= G.DEFERRED_LDS


@pytest.mark.parametrize("ow", [4, 8])
def test_binary_pages_decode_with_the_oracle(ow):
    """P4: the hand-built offsets and values streams are Basic pages the
    reference reads, to the offsets and values the device tests expect."""
    for codec in (O.LZ4, O.SNAPPY):
        for nullable in (False, True):
            pages, offs, vals, valid = G.binary_column(codec, ow, G.ascii_cases(codec)[:6], nullable)
            o, v, m = O.read_binary_column(b"".join(p for p, _ in pages), [(len(p), n) for p, n in pages], nullable, ow)
            assert (o == offs).all() and v == vals
            assert not nullable or (m == valid).all()
            assert all(n >= 600 for _, n in pages)  # a run longer than the 2 KiB of history the device keeps near
