"""``corpus.read_walks``: the host reader of a walk corpus file and the byte definition of ``read_walks_device``.  Literal
expectations for the format's corners, and the round trip with ``save_walks``.  No GPU."""
import numpy as np
import pytest

from pecanpy_amd.corpus import read_walks, save_walks

# (name, the file's bytes, the rows as lists of tokens, the names in first-appearance order, the device reader takes it)
CORPORA = [
    ("plain", b"a b c\nb a\n", [["a", "b", "c"], ["b", "a"]], ["a", "b", "c"], True),
    ("no final newline", b"a b\nc a", [["a", "b"], ["c", "a"]], ["a", "b", "c"], True),
    ("crlf", b"x1 y2\r\ny2 z3 x1\r\n", [["x1", "y2"], ["y2", "z3", "x1"]], ["x1", "y2", "z3"], True),
    ("mixed separators", b"a \t\r  b\t\tc \r\nc\r\rb\n", [["a", "b", "c"], ["c", "b"]], ["a", "b", "c"], True),
    ("leading and trailing separators", b"  a b  \n\t\tb\t\n \n", [["a", "b"], ["b"], []], ["a", "b"], True),
    ("empty lines", b"\na\n\n\nb a\n\n", [[], ["a"], [], [], ["b", "a"], []], ["a", "b"], True),
    ("only newlines", b"\n\n\n", [[], [], []], [], True),
    ("only separators", b" \t \r", [[]], [], True),
    ("one token", b"node", [["node"]], ["node"], True),
    ("punctuation", b"!~ a-b a_b !~\n{x} a-b\n", [["!~", "a-b", "a_b", "!~"], ["{x}", "a-b"]], ["!~", "a-b", "a_b", "{x}"], True),
    ("prefixes", b"1 10 100 10\n100 1\n", [["1", "10", "100", "10"], ["100", "1"]], ["1", "10", "100"], True),
    ("utf-8 name", "Zürich 節點\n節點 a\n".encode("utf-8"), [["Zürich", "節點"], ["節點", "a"]], ["Zürich", "節點", "a"], False),
    ("vertical tab", b"a\x0bb c\n", [["a", "b", "c"]], ["a", "b", "c"], False),
    ("empty file", b"", [], [], False),
]
IDS = [name for name, *_ in CORPORA]


def expected_matrix(rows, names):
    width = max(max((len(r) for r in rows), default=0), 1) + 1
    mat = np.zeros((len(rows), width), dtype=np.uint32)
    for i, r in enumerate(rows):
        mat[i, :len(r)] = [names.index(t) for t in r]
        mat[i, -1] = len(r)
    return mat


@pytest.mark.parametrize("name,data,rows,names,accepted", CORPORA, ids=IDS)
def test_read_walks_literal_corpora(name, data, rows, names, accepted, tmp_path):
    path = tmp_path / "corpus.txt"
    path.write_bytes(data)
    mat, got_names = read_walks(path)
    want = expected_matrix(rows, names)
    assert mat.dtype == np.uint32 and mat.shape == want.shape and np.array_equal(mat, want)
    assert got_names == names and all(type(x) is str for x in got_names)


def test_literal_matrices_cell_by_cell(tmp_path):
    path = tmp_path / "corpus.txt"
    path.write_bytes(b"a b c\r\n\nb\n c  a")
    mat, names = read_walks(path)
    assert names == ["a", "b", "c"]
    assert mat.tolist() == [[0, 1, 2, 3], [0, 0, 0, 0], [1, 0, 0, 1], [2, 0, 0, 2]]
    path.write_bytes(b"")
    mat, names = read_walks(path)
    assert mat.shape == (0, 2) and mat.dtype == np.uint32 and names == []
    path.write_bytes(b"\n\n")
    mat, names = read_walks(path)
    assert mat.tolist() == [[0, 0], [0, 0]] and names == []


def test_node_ids_remap_and_unknown_token(tmp_path):
    path = tmp_path / "corpus.txt"
    path.write_bytes(b"7 3 5\n5 7\n\n3\n")
    mat, names = read_walks(path, node_ids=[3, 5, 7, 9])
    assert names == ["3", "5", "7", "9"]
    assert mat.tolist() == [[2, 0, 1, 3], [1, 2, 0, 2], [0, 0, 0, 0], [0, 0, 0, 1]]
    with pytest.raises(ValueError, match=r"token '5' in line 1 .* 2 node ids"):
        read_walks(path, node_ids=["7", "3"])
    path.write_bytes(b"7 3\n3 7\n7 x9 3\n")
    with pytest.raises(ValueError, match=r"token 'x9' in line 3"):
        read_walks(path, node_ids=["7", "3"])


def ragged(n, walk_length, n_names, seed):
    """uint32[n, walk_length + 2] with zeros behind the row lengths; rows of length 0 and walk_length + 1 among them"""
    rng = np.random.default_rng(seed)
    width = walk_length + 1
    lens = rng.integers(0, width + 1, size=n)
    lens[: min(n, 2)] = [0, width][: min(n, 2)]
    mat = np.zeros((n, walk_length + 2), dtype=np.uint32)
    keep = np.arange(width)[None, :] < lens[:, None]
    mat[:, :width][keep] = rng.integers(0, n_names, size=(n, width), dtype=np.uint32)[keep]
    mat[:, -1] = lens
    return mat


@pytest.mark.parametrize("n,walk_length", [(1, 1), (40, 7), (300, 12), (5, 0), (1, 0)])
def test_round_trip_with_save_walks(n, walk_length, tmp_path):
    ids = ["v%d" % i for i in range(20)] + ["v1x", "Zürich", "9"]   # a name that is a prefix of another, a UTF-8 one
    mat = ragged(n, walk_length, len(ids), seed=n + walk_length)
    path = tmp_path / "corpus.txt"
    save_walks(path, ids, mat)
    got, names = read_walks(path, ids)
    longest = max(int(mat[:, -1].max()), 1)
    want = np.zeros((n, longest + 1), dtype=np.uint32)   # the matrix at width W: the zero cells behind the longest row dropped
    want[:, :longest], want[:, -1] = mat[:, :longest], mat[:, -1]
    assert names == ids and got.dtype == np.uint32 and np.array_equal(got, want)
    # numbered by first appearance instead: the same rows through the names
    free, free_names = read_walks(path)
    assert sorted(free_names) == sorted({ids[i] for r in mat for i in r[: r[-1]]})
    back = np.array([ids.index(x) for x in free_names] + [0], dtype=np.uint32)
    keep = np.arange(longest)[None, :] < want[:, -1:]
    assert np.array_equal(np.where(keep, back[free[:, :-1]], 0), want[:, :-1]) and np.array_equal(free[:, -1], want[:, -1])


def test_rows_of_length_zero_only(tmp_path):
    path = tmp_path / "corpus.txt"
    save_walks(path, ["a"], np.zeros((3, 6), dtype=np.uint32))
    assert path.read_bytes() == b"\n\n\n"
    mat, names = read_walks(path, ["a"])
    assert mat.tolist() == [[0, 0]] * 3 and names == ["a"]
