"""Host side of the dense classes' device edge-list reader: the method exists on every dense class, without a device it is
``read_edg`` bit for bit (the golden matrices of the reference's ``to_dense()``), and ``num_edges`` / ``density`` of an object
that holds a host matrix are what they were."""
import json
import os
import warnings

import numpy as np
import pytest

from pecanpy_amd import _lib, experimental
from pecanpy_amd import pecanpy as node2vec

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "edgelist_dense_cases.json")) as _f:
    DENSE_CASES = json.load(_f)


class _NoDevice:
    """The loaded library with no HIP device visible."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def pw_device_count(self):
        return 0


@pytest.fixture
def no_device(monkeypatch):
    lib = _lib.load()
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice(lib))


def _write(tmp_path, case):
    path = tmp_path / (case["name"] + ".edg")
    with open(path, "w", newline="") as f:
        f.write(case["text"])
    return str(path)


@pytest.mark.parametrize("cls", [node2vec.DenseOTF, experimental.Node2vecPlusPlus], ids=lambda c: c.__name__)
def test_the_dense_classes_have_the_device_reader(cls):
    assert callable(getattr(cls(), "read_edg_device", None))
    assert "pw_edgelist_read_device_ex" in _lib.SYMBOLS and "pw_csr_dev_export_f64" in _lib.SYMBOLS
    assert _lib.EDGELIST_KEEP_F64 == 1


def test_the_fixture_holds_the_shapes_the_dense_build_can_get_wrong():
    by_name = {c["name"]: c for c in DENSE_CASES}
    assert {len(c["ids"]) for c in DENSE_CASES if not c["error"]} >= {1, 64, 65}
    ones = by_name["all_weights_1_00000001"]
    values = np.array(ones["dense_bits"], dtype=np.uint64).view(np.float64)
    assert set(values.tolist()) == {0.0, 1.00000001} and np.float32(1.00000001) == np.float32(1.0)
    assert set(np.array(by_name["all_weights_exactly_one"]["dense_bits"], dtype=np.uint64).view(np.float64).tolist()) == {0.0, 1.0}
    two = np.array(by_name["float32_equal_float64_distinct"]["dense_bits"], dtype=np.uint64).view(np.float64)
    assert {0.1, 0.10000000001} <= set(two.tolist()) and np.float32(0.1) == np.float32(0.10000000001)
    assert by_name["same_pair_other_spelling"]["n_warnings"] == 0 and by_name["same_pair_conflict"]["n_warnings"] == 1
    sinks = by_name["directed_sinks_first_seen_as_id2"]
    mat = np.array(sinks["dense_bits"], dtype=np.uint64).view(np.float64).reshape(len(sinks["ids"]), -1)
    assert (mat != 0).sum(axis=1).min() == 0 and sinks["ids"].index("late") == len(sinks["ids"]) - 1
    assert not by_name["one_line_no_trailing_newline"]["text"].endswith("\n")
    for name in ("ring_64", "ring_65"):     # the last column, the one whose bit is the last of the rows' last word, is in use
        c = by_name[name]
        n = len(c["ids"])
        assert np.any(np.array(c["dense_bits"], dtype=np.uint64).reshape(n, n)[:, n - 1] != 0)


@pytest.mark.parametrize("case", DENSE_CASES, ids=[c["name"] for c in DENSE_CASES])
def test_without_a_device_it_is_read_edg(tmp_path, no_device, case):
    path = _write(tmp_path, case)
    g = node2vec.DenseOTF()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if case["error"]:
            with pytest.raises({"ValueError": ValueError, "IndexError": IndexError}[case["error"]]):
                g.read_edg_device(path, case["weighted"], case["directed"], case["delimiter"])
            return
        g.read_edg_device(path, case["weighted"], case["directed"], case["delimiter"])
    assert g.last_build_stats == {"reader": "host"}
    assert len(caught) == case["n_warnings"], [str(w.message) for w in caught]
    assert list(g.nodes) == case["ids"]
    assert g.data.dtype == np.float64 and g.data.view(np.uint64).ravel().tolist() == case["dense_bits"]
    ref = node2vec.DenseOTF()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref.read_edg(path, case["weighted"], case["directed"], case["delimiter"])
    assert g.data.tobytes() == ref.data.tobytes() and g.nonzero.tobytes() == ref.nonzero.tobytes()


def test_num_edges_and_density_of_a_host_matrix_are_unchanged():
    rng = np.random.default_rng(3)
    mat = np.where(rng.random((37, 37)) < 0.3, rng.random((37, 37)) + 0.5, 0.0)
    g = node2vec.DenseOTF.from_mat(mat, [str(i) for i in range(37)])
    want = (mat != 0).sum()
    assert g.num_edges == want and type(g.num_edges) is type(want)
    assert g.density == want / 37 / 36
    assert g._device_built is None and g._data is not None
    with pytest.raises(ValueError, match="Empty graph"):
        node2vec.DenseOTF().num_edges
