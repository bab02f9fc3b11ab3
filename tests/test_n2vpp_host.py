"""node2vec++ without a GPU: the NumPy restatement (tests/n2vpp_restated.py) against the fixtures generated from the
reference's experimental.Node2vecPlusPlus, and the public surface of pecanpy.experimental."""
import glob
import os
import re

import numpy as np
import pytest

import n2vpp_restated as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "n2vpp", "n2vpp_*.npz")))


def test_fixtures_present():
    names = {os.path.basename(f)[:-4] for f in FIXTURES}
    for want in ("n2vpp_karate_p0.5_q2", "n2vpp_karate_p1_q0.5", "n2vpp_karate_p0.3_q1", "n2vpp_wre_g0.5_p0.7_q0.4",
                 "n2vpp_wdy_g0.0_p0.7_q0.4", "n2vpp_sink_p0.5_q2", "n2vpp_tiny_p0.5_q2", "n2vpp_tiny_p0.5_q0.5"):
        assert want in names


@pytest.mark.parametrize("path", FIXTURES, ids=lambda f: os.path.basename(f)[:-4])
def test_restatement_reproduces_fixture(path):
    z = np.load(path)
    data = z["data"]
    thr = rs.noise_thresholds(data, float(z["gamma"]))
    np.testing.assert_array_equal(thr.view(np.uint32), z["thr"].view(np.uint32))   # (NaN thresholds compare by bits)
    starts = rs.start_array(data.shape[0], int(z["num_walks"]), int(z["seed"]))
    np.testing.assert_array_equal(starts, z["starts"])
    mat = rs.random_walks(data, float(z["p"]), float(z["q"]), float(z["gamma"]), int(z["seed"]), starts, int(z["walk_length"]))
    np.testing.assert_array_equal(mat, z["walks"])
    nonzero = data != 0
    off = z["prob_off"]
    for i, (cur, prev) in enumerate(zip(z["prob_cur"], z["prob_prev"])):
        got = rs.normalized_probs(data, nonzero, float(z["p"]), float(z["q"]), int(cur), None if prev < 0 else int(prev), thr)
        want = z["prob_vals"][off[i]:off[i + 1]]
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def test_tiny_weights_reach_nan_and_inf():
    """The fixtures pin the non-finite cases: all-NaN vectors (q > 1) and vectors with zeros beside NaN (q < 1)."""
    z2 = np.load(os.path.join(REPO, "tests", "golden", "n2vpp", "n2vpp_tiny_p0.5_q2.npz"))
    z05 = np.load(os.path.join(REPO, "tests", "golden", "n2vpp", "n2vpp_tiny_p0.5_q0.5.npz"))

    def vectors(z):
        off = z["prob_off"]
        return [z["prob_vals"][off[i]:off[i + 1]] for i in range(off.size - 1)]

    assert any(np.isnan(v).all() for v in vectors(z2))
    assert any(np.isnan(v).any() and (v == 0).any() for v in vectors(z05))


def test_searchsorted_nan_last():
    """The step's rule: the first k with !(cdf[k] < r)."""
    cdf = np.cumsum(np.array([0.0, np.nan, 0.0]))
    assert np.searchsorted(cdf, 0.3) == 1
    assert np.searchsorted(np.full(3, np.nan), 0.7) == 0


def test_import_paths():
    from pecanpy.experimental import Node2vecPlusPlus
    from pecanpy_amd import experimental
    from pecanpy_amd.graph import DenseGraph
    from pecanpy_amd.pecanpy import Base, DenseOTF

    assert Node2vecPlusPlus is experimental.Node2vecPlusPlus
    assert issubclass(Node2vecPlusPlus, Base) and issubclass(Node2vecPlusPlus, DenseGraph)
    assert not issubclass(Node2vecPlusPlus, DenseOTF)
    g = Node2vecPlusPlus(p=0.5, q=2, gamma=0.5, random_state=3)
    assert isinstance(g, DenseGraph)
    assert g._mode == "Node2vecPlusPlus" and g._always_thresholds
    assert not DenseOTF._always_thresholds


def test_loaders_and_thresholds_without_gpu():
    from pecanpy.experimental import Node2vecPlusPlus

    z = np.load(os.path.join(REPO, "tests", "golden", "n2vpp", "n2vpp_sink_p0.5_q2.npz"))
    g = Node2vecPlusPlus.from_mat(z["data"], [str(i) for i in range(z["data"].shape[0])], p=0.5, q=2)
    assert g.num_nodes == z["data"].shape[0]
    np.testing.assert_array_equal(g.get_noise_thresholds().view(np.uint32), z["thr"].view(np.uint32))


def test_mode_ids_match_header():
    from pecanpy_amd._lib import MODE_IDS

    hdr = open(os.path.join(REPO, "include", "pecanpy_amd.h")).read()
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"(PW_MODE_\w+)\s*=\s*(\d+)", hdr))
    assert enum["PW_MODE_NODE2VEC_PLUSPLUS"] == MODE_IDS["Node2vecPlusPlus"] == 5
    assert enum["PW_MODE_DENSE_OTF"] == MODE_IDS["DenseOTF"]
    assert sorted(enum.values()) == sorted(MODE_IDS.values())
