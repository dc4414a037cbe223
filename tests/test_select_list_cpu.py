"""The host side of selective List reads: StrawboatFile.page_rows (the row
count every nested page starts with, read from the file with 4 bytes a
page) and the new names of the package.  No GPU."""
import numpy as np
import pytest

from tests import sellistgen as G

pa = pytest.importorskip("pyarrow")


def _write(tmp_path, name="lists.sb"):
    """A file with a List<Int64> column on ragged pages and an Int32 column -> (path, list column, flat metas)."""
    import pa_amd

    col = G.column("int64", True, True, "adaptive")
    flat = pa_amd.encode_column(np.arange(5000, dtype=np.int32), None, False, pa_amd.WriteOptions(max_page_size=1024))
    schema = pa.schema([pa.field("l", pa.list_(pa.field("item", pa.int64(), True)), True),
                        pa.field("x", pa.int32(), False)])
    p = tmp_path / name
    p.write_bytes(pa_amd.assemble_file([(col["chunk"], col["metas"]), flat], schema.serialize().to_pybytes()[8:]))
    return p, col, flat[1]


def test_page_rows_of_a_list_column_and_a_flat_column(tmp_path):
    import pa_amd

    p, col, flat_metas = _write(tmp_path)
    with pa_amd.StrawboatFile(p) as f:
        assert [l.depth for l in f.leaves] == [1, 0]
        footer = [m.num_values for m in f.columns[0].pages]
        assert footer == [m.num_values for m in col["metas"]]  # the level counts
        assert f.page_rows(0) == list(G.PAGE_ROWS)
        assert footer != list(G.PAGE_ROWS)
        assert f.page_rows(1) == [m.num_values for m in flat_metas] == [m.num_values for m in f.columns[1].pages]
        assert sum(f.page_rows(1)) == 5000
        with pytest.raises(pa_amd.StrawboatError) as e:
            f.page_rows(2)
        assert e.value.status == pa_amd._native.E_ARG


def test_page_rows_of_a_truncated_file_is_an_error(tmp_path):
    """The footer survives, the data in front of it does not: the list
    column's last page then starts past the end of the file."""
    import pa_amd

    p, col, flat_metas = _write(tmp_path)
    raw = p.read_bytes()
    data = sum(m.length for m in col["metas"])
    footer = raw[data + sum(m.length for m in flat_metas):]  # schema, metas and the tail words
    keep = col["metas"][0].length + col["metas"][1].length + 7  # the first two pages and a little
    cut = tmp_path / "cut.sb"
    cut.write_bytes(raw[:keep] + footer)
    last_start = data - col["metas"][-1].length
    assert last_start > cut.stat().st_size
    with pa_amd.StrawboatFile(cut) as f:
        with pytest.raises(pa_amd.StrawboatError) as e:
            f.page_rows(0)
        assert e.value.status in (pa_amd._native.E_IO, pa_amd._native.E_OUT_OF_SPEC)
        # and the entry point itself, which the footer check above may have kept the call from
        import ctypes

        rows = (ctypes.c_uint64 * len(col["metas"]))()
        st = pa_amd.lib().sb_file_page_rows(f._h, 0, rows, len(col["metas"]))
        assert st == pa_amd._native.E_IO
        assert b"past the end" in pa_amd.lib().sb_file_last_error(f._h)
        assert pa_amd.lib().sb_file_page_rows(f._h, 0, rows, 3) == pa_amd._native.E_ARG


def test_new_names_are_exported():
    import pa_amd

    for name in ("list_page_rows", "read_selected_list", "SelectedListDecoder"):
        assert hasattr(pa_amd, name), name
    assert hasattr(pa_amd.ListColumnDecoder, "select")
    assert hasattr(pa_amd.StrawboatFile, "page_rows") and hasattr(pa_amd.StrawboatFile, "read_selected_list")
    for sym in ("sb_list_page_rows", "sb_file_page_rows", "sb_plan_selected_list_column", "sb_decode_list_selected",
                "sb_plan_selected_leaves"):
        assert sym in pa_amd._native.EXPORTED
        assert hasattr(pa_amd.lib(), sym), sym
