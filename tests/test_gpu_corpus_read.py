"""The walk corpus file read in device memory: ``pw_corpus_read_device`` / ``read_walks_device`` (the kernels of
csrc/corpus_dev.hip.h), ``train_sgns_file`` and ``pecanpy --task train``.  The expectation everywhere is the host definition
``read_walks`` on the same file: the matrix equal as arrays, the names equal as lists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pecanpy_amd import _lib
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.corpus import read_walks, read_walks_device, save_walks_device
from pecanpy_amd.embed import train_sgns_device, train_sgns_file
from test_corpus_read_host import CORPORA, ragged

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
S = 1024   # bytes of text per wavefront in the reader's byte passes (CP_SEG of csrc/corpus_dev.hip.h)


def check(path, data, reader="device", node_ids=None):
    path.write_bytes(data)
    want, want_names = read_walks(path, node_ids)
    d_walks, names = read_walks_device(path, node_ids)
    assert read_walks_device.last_stats["reader"] == reader
    assert d_walks.is_cuda and d_walks.dtype == torch.int32 and d_walks.is_contiguous()
    got = d_walks.cpu().numpy().view(np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert names == want_names
    return want, names


@pytest.mark.parametrize("name,data", [(c[0], c[1]) for c in CORPORA if c[4]], ids=[c[0] for c in CORPORA if c[4]])
def test_hand_written_corpora(name, data, tmp_path):
    want, names = check(tmp_path / "corpus.txt", data)
    st = read_walks_device.last_stats
    assert st["lines"] == want.shape[0] and st["tokens"] == int(want[:, -1].sum()) and st["names"] == len(names)
    assert st["file_bytes"] == len(data)


def filler(n, seed):
    """n bytes of the accepted alphabet: short names over three letters (they repeat), single and double separators, newlines"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abc  \t\r\n", dtype=np.uint8)
    return bytearray(alphabet[rng.choice(alphabet.size, size=n, p=[0.23, 0.23, 0.22, 0.12, 0.08, 0.03, 0.02, 0.07])].tobytes())


def border_file(case, size):
    """`size` bytes with the case's feature at the border between the first two segments (offset S); sizes S - 1, S and S + 1
    cut the same text in front of, on and one byte behind that border"""
    text = filler(2 * S, seed=ord(case))
    if case == "a":     # a token straddles the border
        text[S - 3:S + 3] = b"xyzxyz"
    elif case == "b":   # a token ends on the last byte of a segment, the next segment starts with a separator
        text[S - 4:S + 2] = b" xyz  "
    elif case == "c":   # a segment starts with a newline
        text[S - 2:S + 2] = b"xy\nz"
    elif case == "d":   # a newline closes a segment, a token start opens the next
        text[S - 2:S + 2] = b"x\nyz"
    elif case == "e":   # a run of spaces longer than S: the second segment holds no newline and no token start
        text[9:] = b" " * (2 * S - 9)
    return bytes(text[:size])


@pytest.mark.parametrize("size", [S - 1, S, S + 1, 2 * S], ids=["S-1", "S", "S+1", "2S"])
@pytest.mark.parametrize("case", "abcde")
def test_segment_borders(case, size, tmp_path):
    data = border_file(case, size)
    assert len(data) == size
    check(tmp_path / "corpus.txt", data)


def test_blank_segment_between_two_tokens(tmp_path):
    check(tmp_path / "corpus.txt", b"ab cd\nef" + b" " * (2 * S + 100) + b"gh ab\n")


def test_one_line_of_5000_tokens(tmp_path):
    data = b" ".join(b"t%d" % (i * 13 % 700) for i in range(5000)) + b"\n"
    assert len(data) > 16 * S and data.count(b"\n") == 1
    want, names = check(tmp_path / "corpus.txt", data)
    assert want.shape == (1, 5001) and want[0, -1] == 5000 and len(names) == 700


def test_segment_with_more_than_64_lines(tmp_path):
    rng = np.random.default_rng(11)
    pieces = [b"a\n", b"\n", b"b\n", b"c a\n", b"\n\n", b"d\n"]
    data = b"".join(pieces[i] for i in rng.integers(0, len(pieces), size=1200))
    assert len(data) > 2 * S and min(data[k:k + S].count(b"\n") for k in range(0, len(data) - S, S)) > 64
    check(tmp_path / "corpus.txt", data)


def test_many_names_few_tokens_each(tmp_path):
    rng = np.random.default_rng(5)
    label = rng.permutation(100000)[:3000]
    order = list(range(3000)) + list(range(1000, 3000))   # name k >= 1000 appears at token k and at token k + 2000
    tokens = [b"n%d" % label[k] for k in order]
    lines, at = [], 0
    while at < len(tokens):
        n = int(rng.integers(1, 41))
        lines.append(b" ".join(tokens[at:at + n]))
        at += n
    want, names = check(tmp_path / "corpus.txt", b"\n".join(lines) + b"\n")
    assert names == ["n%d" % label[k] for k in range(3000)]
    flat = np.concatenate([row[: row[-1]] for row in want])
    assert flat.size == 5000 and np.array_equal(flat, np.array(order))


def test_round_trip_with_the_device_writer(tmp_path):
    ids = ["v%d" % i for i in range(30)] + ["v1x", "v1xy", "node-9", "9"]   # "v1" < "v1x" < "v1xy": prefixes of one another
    mat = ragged(300, 7, len(ids), seed=4)
    path = tmp_path / "corpus.txt"
    d_mat = torch.from_numpy(mat.view(np.int32)).cuda()
    save_walks_device(path, ids, d_mat)
    d_back, names = read_walks_device(path, node_ids=ids)
    assert read_walks_device.last_stats["reader"] == "device" and names == ids
    assert d_back.dtype == torch.int32 and d_back.is_contiguous() and torch.equal(d_back, d_mat)
    want, _ = read_walks(path, ids)
    assert np.array_equal(want, mat)


def test_unknown_token_is_the_host_readers_error(tmp_path):
    path = tmp_path / "corpus.txt"
    path.write_bytes(b"7 3\n3 7\n\n7 x9 3 y\ny\n")
    for reader in (read_walks, read_walks_device):
        with pytest.raises(ValueError, match=r"token 'x9' in line 4 of the corpus is not among the 2 node ids"):
            reader(path, ["7", "3"])


@pytest.mark.parametrize("data", [b"a \xc2\x80b c\nc a\n", b"a\x0bb c\nc\n", b"a\x00b c\nc\n", b"a \x7f c\nc\n", b""],
                         ids=["0x80", "vertical tab", "NUL", "0x7F", "empty file"])
def test_declined_files_go_through_the_host_reader(data, tmp_path):
    check(tmp_path / "corpus.txt", data, reader="host")


def test_missing_file(tmp_path):
    with pytest.raises(FileNotFoundError):
        read_walks_device(tmp_path / "nope.txt")
    with pytest.raises(FileNotFoundError):
        train_sgns_file(tmp_path / "nope.txt")


def test_export_agrees_with_fill(tmp_path):
    path = tmp_path / "corpus.txt"
    path.write_bytes(border_file("a", 2 * S))
    lib = _lib.load()
    h, ids, st = C.c_void_p(), C.c_void_p(), _lib.PwCorpusDevStats()
    assert lib.pw_corpus_read_device(os.fsencode(path), 0, C.byref(h), C.byref(ids), C.byref(st)) == _lib.EDGELIST_OK
    try:
        dims = [C.c_uint64(0) for _ in range(3)]
        _lib.check(lib.pw_corpus_dev_shape(h, *[C.byref(d) for d in dims]))
        n_rows, width, n_tokens = (int(d.value) for d in dims)
        want, names = read_walks(path)
        assert (n_rows, width) == want.shape and n_tokens == int(want[:, -1].sum()) == st.tokens
        assert st.lines == n_rows and st.names == len(names) and st.file_bytes == 2 * S
        exported = np.full((n_rows, width), 0xFFFFFFFF, dtype=np.uint32)
        _lib.check(lib.pw_corpus_dev_export(h, C.c_void_p(exported.ctypes.data)))
        d_out = torch.full((n_rows, width), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.pw_corpus_dev_fill(h, C.c_void_p(d_out.data_ptr())))
        assert np.array_equal(exported, want) and np.array_equal(d_out.cpu().numpy().view(np.uint32), exported)
    finally:
        lib.pw_corpus_dev_destroy(h)
        lib.pw_edgelist_ids_destroy(ids)


def _karate():
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    return k["indptr"], k["indices"], k["data"], [str(i) for i in k["ids"]]


def _karate_graph(seed):
    indptr, indices, data, ids = _karate()
    return node2vec.SparseOTF.from_csr(indptr, indices, data, node_ids=ids, p=0.5, q=2, random_state=seed)


def test_trainer_from_the_file_equals_trainer_from_the_matrix(tmp_path):
    ids = _karate()[3]
    path = tmp_path / "walks.txt"
    _karate_graph(seed=3).walks_to_file(path, 2, 10)
    d_orig = _karate_graph(seed=3)._device_walks(2, 10)
    d_read, names = read_walks_device(path, node_ids=ids)
    assert read_walks_device.last_stats["reader"] == "device" and names == ids
    assert d_read.shape == (68, 12) and torch.equal(d_read, d_orig)
    kw = dict(dim=16, seed=7, workers=1)
    from_file = train_sgns_device(d_read, 34, **kw)
    from_matrix = train_sgns_device(d_orig, 34, **kw)
    assert torch.equal(from_file, from_matrix)   # bit for bit: workers=1 is the deterministic form, the matrices are equal

    names, d_vec = train_sgns_file(path, **kw)
    first_appearance = read_walks(path)[1]
    assert names == first_appearance and sorted(names) == sorted(ids)
    assert d_vec.is_cuda and d_vec.dtype == torch.float32 and d_vec.shape == (34, 16) and bool(torch.isfinite(d_vec).all())
    st = train_sgns_file.last_stats
    assert st["read"]["reader"] == "device" and st["read"]["lines"] == 68 and st["read"]["tokens"] == 68 * 11
    assert st["train"]["trained_pairs"] > 0


def test_train_sgns_file_refuses_what_it_cannot_train(tmp_path):
    path = tmp_path / "corpus.txt"
    path.write_bytes(b"")
    with pytest.raises(ValueError, match="without lines"):
        train_sgns_file(path)
    path.write_bytes(b"a " * 8193 + b"\n")
    with pytest.raises(ValueError, match="8193 tokens exceeds the trainer's walk length limit"):
        train_sgns_file(path)


def test_cli_task_train_in_a_fresh_process(tmp_path):
    indptr, indices, _, ids = _karate()
    edg = tmp_path / "karate.edg"
    with open(edg, "w") as f:
        for u in range(34):
            for v in indices[indptr[u]:indptr[u + 1]]:
                if u < v:
                    f.write(f"{ids[u]}\t{ids[v]}\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PECANPY_AMD_DUMP_WALKS", None)

    def run(*args):
        res = subprocess.run([sys.executable, "-W", "ignore", "-m", "pecanpy_amd.cli"] + [str(a) for a in args], env=env,
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        return res.stdout

    walks, emb, npz = tmp_path / "walks.txt", tmp_path / "karate.emb", tmp_path / "karate.npz"
    run("--input", edg, "--output", walks, "--task", "walks", "--mode", "SparseOTF", "--p", 0.5, "--q", 2, "--random_state", 1,
        "--num-walks", 4, "--walk-length", 15)
    out = run("--input", walks, "--output", emb, "--task", "train", "--dimensions", 8, "--window-size", 5, "--epochs", 2,
              "--random_state", 1, "--verbose")
    assert "corpus read by the device reader" in out
    lines = emb.read_text().split("\n")
    assert lines[0] == "34 8" and lines[-1] == "" and len(lines) == 36
    rows = [ln.split(" ") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == read_walks(walks)[1]
    assert all(len(r) == 9 for r in rows) and np.isfinite(np.array([[float(x) for x in r[1:]] for r in rows])).all()
    run("--input", walks, "--output", npz, "--task", "train", "--dimensions", 8, "--random_state", 1)
    z = np.load(npz)
    assert z["IDs"].tolist() == read_walks(walks)[1] and z["data"].shape == (34, 8) and z["data"].dtype == np.float32
    assert np.isfinite(z["data"]).all()
