"""The embedding file written from device memory: ``pw_vectors_write_text_device`` / ``save_word2vec_format_device`` (the
kernels of csrc/emb_text.hip.h), ``Base.embed_to_file``, and the command line's text output.  The expectation everywhere is
Python itself -- ``"%.6f" % float(x)``, and for whole files ``save_word2vec_format`` on the same data -- and every
comparison is byte equality."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from emb_text_cases import adversarial_values, assert_equals_python, selftest_f6
from pecanpy_amd import _lib
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.embed import save_word2vec_format, save_word2vec_format_device
from pecanpy_amd.engine import PwError

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SHAPES = [(1, 1), (1, 512), (5, 3), (257, 64), (300, 65), (100, 130), (64, 1000), (4097, 128)]
SPECIAL_NAMES = ["Zürich", "節點", "x", "L" * 300]          # two- and three-byte characters, one byte, 300 bytes


def make_vectors(n, dim, seed=0):
    """N(0, 0.3) with the adversarial values scattered in (as many as fit), float32[n, dim]."""
    rng = np.random.default_rng(seed)
    vec = (rng.standard_normal((n, dim)) * 0.3).astype(np.float32)
    adv = rng.permutation(adversarial_values())[: n * dim]
    vec.reshape(-1)[rng.choice(n * dim, size=adv.size, replace=False)] = adv
    return vec


def make_names(n):
    names = [("n%d" % i) * (1 + i % 4) for i in range(n)]
    for j, s in enumerate(SPECIAL_NAMES):
        names[(j * 37) % n] = s
    return names


def on_device(vec):
    import torch

    return torch.from_numpy(vec).cuda()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """The (4097, 128) case and its reference file, shared by the tests that need them."""
    vec, names = make_vectors(4097, 128, seed=7), make_names(4097)
    path = tmp_path_factory.mktemp("emb") / "want.emb"
    save_word2vec_format(path, names, vec)
    return vec, names, path.read_bytes()


def expected_chunks(file_bytes, budget):
    """Consecutive rows while their text fits the budget."""
    rows = [len(r) + 1 for r in file_bytes.split(b"\n")[1:-1]]
    assert max(rows) <= budget
    chunks, used = 1, 0
    for r in rows:
        if used + r > budget:
            chunks, used = chunks + 1, 0
        used += r
    return chunks


def test_selftest_on_the_device_equals_the_host_build_and_python():
    lib = _lib.load()
    rng = np.random.default_rng(20240613)
    x = np.concatenate([adversarial_values(),
                        rng.integers(0, 2 ** 32, size=1_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    chars, lens = selftest_f6(lib, x, on_device=1)
    host_chars, host_lens = selftest_f6(lib, x, on_device=0)
    assert np.array_equal(lens, host_lens) and np.array_equal(chars, host_chars)
    assert_equals_python(x, chars, lens)


@pytest.mark.parametrize("n,dim", SHAPES)
def test_whole_files_equal_the_host_writer(n, dim, tmp_path):
    vec, names = make_vectors(n, dim, seed=n + dim), make_names(n)
    if n >= 5:
        assert all(s in names for s in SPECIAL_NAMES)
    want, got = tmp_path / "want.emb", tmp_path / "got.emb"
    d_vec = on_device(vec)
    save_word2vec_format(want, names, d_vec.cpu().numpy())
    save_word2vec_format_device(got, names, d_vec)
    assert got.read_bytes() == want.read_bytes()
    st = save_word2vec_format_device.last_stats
    assert st["bytes"] == os.path.getsize(want) and st["chunks"] == 1 and st["format_ms"] > 0
    # node names given as a NumPy array (what the graph classes hold after reading an .npz)
    save_word2vec_format_device(got, np.array(names), d_vec)
    assert got.read_bytes() == want.read_bytes()
    assert np.array_equal(d_vec.cpu().numpy().view(np.uint32), vec.view(np.uint32))   # the vectors are read, never written


@pytest.mark.parametrize("budget", [65536, 1])
def test_chunks_leave_the_bytes_unchanged(budget, big, tmp_path, monkeypatch):
    vec, names, want = big
    monkeypatch.setenv("PECANPY_AMD_EMB_CHUNK_BYTES", str(budget))
    got = tmp_path / "got.emb"
    save_word2vec_format_device(got, names, on_device(vec))
    assert got.read_bytes() == want
    # a budget below what one row can take is raised to that: the longest name, 48 bytes per component, the newline
    effective = max(budget, 300 + 128 * 48 + 1)
    chunks = expected_chunks(want, effective)
    print(f"budget {budget} -> {effective}: {chunks} chunks")
    assert 1 < chunks and save_word2vec_format_device.last_stats["chunks"] == chunks
    assert save_word2vec_format_device.last_stats["bytes"] == len(want)


def _write_text_host(path, names, vec):
    blob = b"".join(s.encode("utf-8") for s in names)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(s.encode("utf-8")) for s in names], out=off[1:])
    st = _lib.PwEmbWriteStats()
    rc = _lib.load().pw_vectors_write_text(0, C.c_void_p(vec.ctypes.data), vec.shape[0], vec.shape[1], blob,
                                           C.c_void_p(off.ctypes.data), os.fsencode(path), C.byref(st))
    return rc, st.as_dict()


def test_host_pointer_entry_equals_the_device_entry(big, tmp_path):
    vec, names, want = big
    got = tmp_path / "got.emb"
    rc, st = _write_text_host(got, names, vec)
    assert rc == 0 and got.read_bytes() == want and st["bytes"] == len(want)


def test_embed_to_file_equals_embed_array_and_the_host_writer(tmp_path):
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    g = node2vec.SparseOTF.from_csr(k["indptr"], k["indices"], k["data"], node_ids=list(k["ids"]), p=1, q=0.5, random_state=0)
    kw = dict(dim=12, num_walks=6, walk_length=25, window_size=4, epochs=2, workers=1)
    want, got = tmp_path / "want.emb", tmp_path / "got.emb"
    g.embed_to_file(got, **kw)
    st = g.last_embed_stats
    assert st["vectors_host_bytes"] == 0 and st["walk_matrix_host_bytes"] == 0 and st["wavefronts"] == 1
    assert st["write_call_ms"] > 0 and st["chunks"] == 1 and st["bytes"] == os.path.getsize(got) and st["train_ms"] > 0
    save_word2vec_format(want, g.nodes, g.embed_array(**kw))
    assert got.read_bytes() == want.read_bytes()
    assert "download_ms" in g.last_embed_stats                        # embed_array's own record is unchanged


def test_cli_text_output_in_a_fresh_process(tmp_path):
    """A fresh child process: edge list -> ``--output x.emb``, whichever writer the command line uses (MEASUREMENTS.md,
    "Embedding file from device memory").  Its trainer is hogwild (not repeatable bit for bit), so the file is compared in
    structure: header, row count, names, every field a ``%.6f`` number."""
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    indptr, indices, ids = k["indptr"], k["indices"], k["ids"]
    edg, out = tmp_path / "karate.edg", tmp_path / "karate.emb"
    with open(edg, "w") as f:
        for u in range(34):
            for v in indices[indptr[u]:indptr[u + 1]]:
                if u < v:
                    f.write(f"{ids[u]}\t{ids[v]}\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PECANPY_AMD_DUMP_WALKS", None)
    res = subprocess.run([sys.executable, "-W", "ignore", "-m", "pecanpy_amd.cli", "--input", str(edg), "--output", str(out),
                          "--mode", "SparseOTF", "--p", "1", "--q", "0.5", "--random_state", "1", "--num-walks", "10",
                          "--walk-length", "20", "--dimensions", "16", "--epochs", "2", "--window-size", "5"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    data = out.read_bytes()
    assert data.endswith(b"\n") and b"\r" not in data
    lines = data.decode("utf-8").split("\n")[:-1]
    assert lines[0] == "34 16" and len(lines) == 35
    rows = [ln.split(" ") for ln in lines[1:]]
    assert sorted(r[0] for r in rows) == sorted(str(i) for i in ids)
    number = re.compile(r"-?\d+\.\d{6}")
    assert all(len(r) == 17 and all(number.fullmatch(x) for x in r[1:]) for r in rows)
    vec = np.array([[float(x) for x in r[1:]] for r in rows])
    assert np.abs(vec).max() > 0                                       # vectors, not zeros


def test_bad_arguments_are_errors_and_the_next_call_succeeds(big, tmp_path):
    vec, names, want = big
    d_vec = on_device(vec)
    with pytest.raises(PwError, match="cannot open .*No such file or directory"):
        save_word2vec_format_device(tmp_path / "no_such_directory" / "x.emb", names, d_vec)
    refused = tmp_path / "refused.emb"                                 # real device tensors of the wrong kind
    with pytest.raises(ValueError, match="must be contiguous"):
        save_word2vec_format_device(refused, names, d_vec[:, ::2])
    with pytest.raises(ValueError, match="must be float32, not torch.float64"):
        save_word2vec_format_device(refused, names, d_vec.double())
    with pytest.raises(ValueError, match="4096 node names for 4097 rows"):
        save_word2vec_format_device(refused, names[:-1], d_vec)
    assert not refused.exists()
    lib = _lib.load()
    off = np.arange(4, dtype=np.uint64)
    off[2] = 0                                                        # offsets that do not ascend
    small = on_device(vec[:3])
    path = os.fsencode(tmp_path / "bad.emb")
    for n_rows, dim, offsets in ((3, 128, off), (0, 128, off), (3, 0, off)):
        rc = lib.pw_vectors_write_text_device(0, C.c_void_p(small.data_ptr()), n_rows, dim, b"abc", C.c_void_p(offsets.ctypes.data),
                                              path, None)
        assert rc == -1, (n_rows, dim)                                 # PW_ERR_INVALID
    assert b"do not ascend" in lib.pw_last_error() or b"must be positive" in lib.pw_last_error()
    got = tmp_path / "got.emb"
    save_word2vec_format_device(got, names, d_vec)
    assert got.read_bytes() == want
