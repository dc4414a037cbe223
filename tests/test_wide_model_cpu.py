"""tests/widegen.py pinned where the oracle can see it: at W = 8 the model's
pages equal oracle.write_page's for signed int64 columns, byte for byte, and
the oracle reads them back -- every option set, both nullabilities, page sizes
on either side of the sampler's threshold, every data shape."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import widegen as G
from tests.widecases import OPTS, SHAPES, SIZES, shape


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_model_equals_oracle_at_w8(opt, nullable):
    rng = np.random.default_rng(sum(map(ord, opt)) + nullable)
    for n in SIZES:
        for kind in SHAPES:
            vals, valid = shape(kind, n, 8, rng)
            if not nullable:
                valid = None
            o = O.WriteOptions.make(**OPTS[opt])
            arr = G.as_array(vals, 8)
            want = O.write_page(arr, valid, nullable, o)
            got = G.write_page(vals, valid, nullable, o, W=8)
            assert got == want, (opt, nullable, n, kind, got[:16].hex(), want[:16].hex())
            back, bv = O.read_page(got, n, np.int64, nullable)
            raw, mv = G.read_page(got, n, 8, nullable)
            assert raw == back.tobytes(), (opt, n, kind)
            if nullable:
                assert (bv == mv).all()


def test_sampler_is_splitmix64():
    r = G.Rng(0)  # the reference vector of splitmix64 from seed 0
    assert [r.next() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_as_i64_truncates():
    assert G.as_i64((1 << 64) + 5) == 5
    assert G.as_i64(-1) == -1
    assert G.as_i64((1 << 63)) == -(1 << 63)


def test_reader_classes():
    W = 16
    with pytest.raises(G.Malformed) as e:
        G.read_page(G.stream(G.BITPACKING, b"\0" * 64, 128, W), 128, W)
    assert e.value.code == G.E_OUT_OF_SPEC
    with pytest.raises(G.Malformed) as e:
        G.read_page(G.none_stream([1, 2, 3], W)[:-1], 3, W)
    assert e.value.code == G.E_IO
    with pytest.raises(G.Malformed) as e:
        G.read_page(G.stream(G.LZ4, b"\xff\xff\xff", 3, W), 3, W)
    assert e.value.code == G.E_CODEC
