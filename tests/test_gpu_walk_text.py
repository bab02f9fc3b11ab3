"""The walk corpus file written from device memory: ``pw_walks_write_text_device`` / ``save_walks_device`` (the kernels of
csrc/walk_text.hip.h), ``Base.walks_to_file`` and ``pecanpy --task walks``.  The expectation everywhere is the host:
``save_walks`` on the same matrix, and for real walks ``cli._dump_walks`` of ``simulate_walks`` -- every comparison is byte
equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from pecanpy_amd import _lib, cli
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.corpus import save_walks, save_walks_device
from pecanpy_amd.engine import PwError

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
# tokens per full row 2, 4, 63, 64, 65, 130 and 81: both sides of the 64-lane trip, three trips; and walk_length 0: start nodes
SHAPES = [(1, 1), (5, 3), (257, 62), (300, 63), (100, 64), (64, 129), (4097, 80), (3, 0)]
STAGE = 3072                                  # bytes of text one trip passes through LDS at once (EMB_PIECE)
N_NAMES, ZURICH, NODE, EMPTY, ONE, LONG, HUGE = 50, 7, 11, 13, 14, 17, 19


def make_names():
    """50 names: short ASCII ones, two- and three-byte characters, the empty string, one byte, 300 bytes, and 5 000 bytes --
    longer than the stage."""
    names = [("n%d" % i) * (1 + i % 4) for i in range(N_NAMES)]
    names[ZURICH], names[NODE], names[EMPTY], names[ONE], names[LONG], names[HUGE] = "Zürich", "節點", "", "x", "L" * 300, "H" * 5000
    return names


def make_walks(n, walk_length, seed):
    """uint32[n, walk_length + 2]: random names (the 5 000-byte one rarely), random lengths in [0, walk_length + 1]; as far as
    n and the width allow: rows of length 0, 1 and walk_length + 1, a row with the 5 000-byte name twice in a row and as last
    token, and two rows whose first trip is exactly the stage and one byte more.  Cells behind the length hold 0xffffffff."""
    rng = np.random.default_rng(seed)
    width = walk_length + 1
    others = np.array([i for i in range(N_NAMES) if i != HUGE], dtype=np.uint32)
    tok = others[rng.integers(0, others.size, size=(n, width))]
    tok[rng.random((n, width)) < 0.002] = HUGE
    lens = rng.integers(0, width + 1, size=n).astype(np.uint32)
    for row, forced in enumerate((0, 1, width)):
        if row < n:
            lens[row] = forced
    if n > 3 and width >= 3:
        lens[3] = width
        tok[3, 0] = tok[3, 1] = tok[3, width - 1] = HUGE
    if n > 5 and width >= 64:
        for row, ones in ((4, 8), (5, 9)):          # 10 * 301 + 2 * ones + (54 - ones) = 3072, 3073 bytes in the first 64 tokens
            lens[row] = width
            tok[row, :64] = [LONG] * 10 + [ONE] * ones + [EMPTY] * (54 - ones)
    mat = np.full((n, walk_length + 2), 0xFFFFFFFF, dtype=np.uint32)
    keep = np.arange(width)[None, :] < lens[:, None]
    mat[:, :width][keep] = tok[keep]
    mat[:, -1] = lens
    return mat


def on_device(mat):
    import torch

    return torch.from_numpy(np.ascontiguousarray(mat).view(np.int32)).cuda()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """The (4097, 80) case and its reference file, shared by the tests that need them."""
    mat, names = make_walks(4097, 80, seed=7), make_names()
    path = tmp_path_factory.mktemp("walks") / "want.txt"
    save_walks(path, names, mat)
    return mat, names, path.read_bytes()


def expected_chunks(file_bytes, budget):
    """Consecutive rows while their text fits the budget."""
    rows = [len(r) + 1 for r in file_bytes.split(b"\n")[:-1]]
    assert max(rows) <= budget
    chunks, used = 1, 0
    for r in rows:
        if used + r > budget:
            chunks, used = chunks + 1, 0
        used += r
    return chunks


def test_the_threshold_rows_sit_on_both_sides_of_the_stage():
    mat, names = make_walks(100, 64, seed=1), make_names()
    first_trip = [sum(len(names[t].encode()) + 1 for t in mat[row, :64]) for row in (4, 5)]
    assert first_trip == [STAGE, STAGE + 1]


@pytest.mark.parametrize("n,walk_length", SHAPES)
def test_whole_files_equal_the_host_writer(n, walk_length, tmp_path):
    mat, names = make_walks(n, walk_length, seed=n + walk_length), make_names()
    lens = mat[:, -1]
    if n >= 5:
        assert {0, 1, walk_length + 1} <= set(lens.tolist()) and (mat[3, :2] == HUGE).all() and mat[3, walk_length] == HUGE
    want, got = tmp_path / "want.txt", tmp_path / "got.txt"
    d_mat = on_device(mat)
    save_walks(want, names, mat)
    save_walks_device(got, names, d_mat)
    assert got.read_bytes() == want.read_bytes()
    st = save_walks_device.last_stats
    print(st)
    assert st["bytes"] == os.path.getsize(want) and st["chunks"] == 1 and st["format_ms"] > 0
    assert st["rows"] == n and st["tokens"] == int(lens.sum(dtype=np.uint64))
    # node names given as a NumPy array (what the graph classes hold after reading an .npz)
    save_walks_device(got, np.array(names), d_mat)
    assert got.read_bytes() == want.read_bytes()
    assert np.array_equal(d_mat.cpu().numpy().view(np.uint32), mat)              # the matrix is read, never written


@pytest.mark.parametrize("budget", [65536, 1, 1 << 20])   # the first two are raised to the same row maximum, the third is not
def test_chunks_leave_the_bytes_unchanged(budget, big, tmp_path, monkeypatch):
    mat, names, want = big
    monkeypatch.setenv("PECANPY_AMD_WALKS_CHUNK_BYTES", str(budget))
    got = tmp_path / "got.txt"
    save_walks_device(got, names, on_device(mat))
    assert got.read_bytes() == want
    # a budget below the longest possible row is raised to that: walk_length + 1 times the longest name and its separator
    effective = max(budget, 81 * 5001)
    chunks = expected_chunks(want, effective)
    print(f"budget {budget} -> {effective}: {chunks} chunks of {len(want)} bytes")
    assert 1 < chunks and save_walks_device.last_stats["chunks"] == chunks
    assert save_walks_device.last_stats["bytes"] == len(want)


def _write_text_host(path, names, mat):
    blob = b"".join(s.encode("utf-8") for s in names)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(s.encode("utf-8")) for s in names], out=off[1:])
    st = _lib.PwWalksWriteStats()
    rc = _lib.load().pw_walks_write_text(0, C.c_void_p(mat.ctypes.data), mat.shape[0], mat.shape[1] - 2, blob,
                                         C.c_void_p(off.ctypes.data), len(names), os.fsencode(path), C.byref(st))
    return rc, st.as_dict()


def test_host_pointer_entry_equals_the_device_entry(big, tmp_path):
    mat, names, want = big
    got = tmp_path / "got.txt"
    rc, st = _write_text_host(got, names, mat)
    assert rc == 0 and got.read_bytes() == want
    assert st["bytes"] == len(want) and st["rows"] == 4097 and st["tokens"] == int(mat[:, -1].sum(dtype=np.uint64))


def _karate():
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    return k["indptr"], k["indices"], k["data"], [str(i) for i in k["ids"]]


def _karate_graph(mode, seed):
    indptr, indices, data, ids = _karate()
    kw = dict(p=0.5, q=2, random_state=seed)
    if mode == "DenseOTF":
        dense = np.zeros((34, 34))
        dense[np.repeat(np.arange(34), np.diff(indptr.astype(np.int64))), indices] = data
        return node2vec.DenseOTF.from_mat(dense, ids, **kw)
    return getattr(node2vec, mode).from_csr(indptr, indices, data, node_ids=ids, **kw)


@pytest.mark.parametrize("mode", ["SparseOTF", "DenseOTF", "PreComp"])
def test_walks_to_file_equals_the_dump_of_simulate_walks(mode, tmp_path):
    want, got = tmp_path / "want.txt", tmp_path / "got.txt"
    g = _karate_graph(mode, seed=3)
    g.walks_to_file(got, 6, 25)
    st = g.last_corpus_stats
    assert st["walk_matrix_host_bytes"] == 0 and st["rows"] == 6 * 34 and st["tokens"] == 6 * 34 * 26
    assert st["bytes"] == os.path.getsize(got) and st["write_call_ms"] > 0 and st["walk_ms"] > 0
    cli._dump_walks(want, _karate_graph(mode, seed=3).simulate_walks(6, 25))
    assert got.read_bytes() == want.read_bytes()


def test_walks_that_end_in_sinks_give_shorter_lines(tmp_path):
    # 3 and 7 have no way out, 8 has no edge at all; vertex i is id i
    edges = np.array([[0, 1, 2, 4, 4, 5, 6, 6, 1, 2], [1, 2, 3, 0, 5, 4, 7, 0, 4, 6]], dtype=np.int64)
    ids = ["v%d" % i for i in range(9)]
    kw = dict(num_nodes=9, directed=True, node_ids=ids, p=0.5, q=2, random_state=5)
    want, got = tmp_path / "want.txt", tmp_path / "got.txt"
    g = node2vec.SparseOTF.from_edge_index(edges, **kw)
    g.walks_to_file(got, 5, 12)
    assert g.last_corpus_stats["walk_matrix_host_bytes"] == 0 and g.last_corpus_stats["rows"] == 45
    cli._dump_walks(want, node2vec.SparseOTF.from_edge_index(edges, **kw).simulate_walks(5, 12))
    assert got.read_bytes() == want.read_bytes()
    tokens = [len(line.split(" ")) for line in got.read_text().splitlines()]
    assert min(tokens) == 1 and max(tokens) <= 13 and g.last_corpus_stats["tokens"] == sum(tokens) < 45 * 13


def test_cli_task_walks_in_a_fresh_process_equals_the_dump_route(tmp_path):
    indptr, indices, _, ids = _karate()
    edg = tmp_path / "karate.edg"
    with open(edg, "w") as f:
        for u in range(34):
            for v in indices[indptr[u]:indptr[u + 1]]:
                if u < v:
                    f.write(f"{ids[u]}\t{ids[v]}\n")
    args = ["--input", str(edg), "--mode", "SparseOTF", "--p", "0.5", "--q", "2", "--random_state", "1", "--num-walks", "4",
            "--walk-length", "15"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PECANPY_AMD_DUMP_WALKS", None)
    out = {}
    for route, extra, extra_env in (("task", ["--task", "walks"], {}), ("dump", [], {"PECANPY_AMD_DUMP_WALKS": "1"})):
        out[route] = tmp_path / f"{route}.txt"
        res = subprocess.run([sys.executable, "-W", "ignore", "-m", "pecanpy_amd.cli", "--output", str(out[route])] + args + extra,
                             env=dict(env, **extra_env), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
    data = out["task"].read_bytes()
    assert data == out["dump"].read_bytes()
    lines = data.decode("utf-8").split("\n")
    assert lines[-1] == "" and len(lines) == 4 * 34 + 1 and all(len(ln.split(" ")) == 16 for ln in lines[:-1])


def test_bad_input_is_an_error_and_the_next_call_succeeds(big, tmp_path):
    mat, names, want = big
    small = make_walks(40, 9, seed=2)
    got = tmp_path / "got.txt"
    bad = small.copy()
    bad[6, :5], bad[6, -1] = [1, 2, 3, N_NAMES, 4], 5                  # a token without a name, in front of the length
    with pytest.raises(PwError, match=r"node index 50 at position 3 of row 6 outside the 50 names"):
        save_walks_device(got, names, on_device(bad))
    assert got.read_bytes() == b""                                     # refused before any text was made
    bad = small.copy()
    bad[8, -1] = 9 + 2                                                 # a length beyond the row
    with pytest.raises(PwError, match=r"row length 11 in row 8 exceeds walk_length \+ 1 = 10"):
        save_walks_device(got, names, on_device(bad))
    assert got.read_bytes() == b""
    refused = tmp_path / "refused.txt"                                 # real device tensors of the wrong kind
    d_mat = on_device(mat)
    with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
        save_walks_device(refused, names, d_mat[:, ::2])
    with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
        save_walks_device(refused, names, d_mat.long())
    with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
        save_walks_device(refused, names, mat)
    assert not refused.exists()
    with pytest.raises(PwError, match="cannot open .*No such file or directory"):
        save_walks_device(tmp_path / "no_such_directory" / "x.txt", names, d_mat)
    save_walks_device(got, names, d_mat[:0])                           # no walks: the empty file
    assert got.read_bytes() == b"" and save_walks_device.last_stats["rows"] == 0
    save_walks_device(got, names, d_mat)
    assert got.read_bytes() == want
