"""The walk corpus file on the host (no GPU): ``pecanpy_amd.corpus.save_walks`` is the byte definition of the format -- what
``cli._dump_walks`` writes for the ID lists ``Base._map_walk`` makes of the same rows -- and ``--task walks`` is a task of the
command line that leaves the conversion tasks as they were."""
import numpy as np
import pytest

from pecanpy_amd import cli
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.corpus import save_walks

N_NAMES = 23
NAMES = {
    "str": ["n%d" % i for i in range(N_NAMES)],
    "numpy": np.array(["gene%d" % (i * i) for i in range(N_NAMES)]),
    "int": [1000 - 7 * i for i in range(N_NAMES)],
    "multibyte": ["Zürich", "節點", "", "ß" * 40] + ["ü%d" % i for i in range(N_NAMES - 4)],
}


def ragged_matrix(n_walks, walk_length, n_names, seed):
    """Random tokens, random lengths in [0, walk_length + 1] with 0, 1 and the full length present, garbage behind the length."""
    rng = np.random.default_rng(seed)
    mat = rng.integers(0, n_names, size=(n_walks, walk_length + 2), dtype=np.uint32)
    lens = rng.integers(0, walk_length + 2, size=n_walks, dtype=np.uint32)
    lens[:3] = [0, 1, walk_length + 1]
    mat[:, -1] = lens
    mat[np.arange(walk_length + 2)[None, :] >= lens[:, None]] = 0xFFFFFFFF
    mat[:, -1] = lens
    return mat


def through_id_lists(path, names, mat):
    g = node2vec.SparseOTF()
    g.set_node_ids(names)
    cli._dump_walks(path, [[str(x) for x in g._map_walk(r)] for r in mat])   # (_map_walk slices before it looks up)


@pytest.mark.parametrize("kind", sorted(NAMES))
def test_save_walks_equals_dump_walks_of_the_mapped_rows(kind, tmp_path, monkeypatch):
    names = NAMES[kind]
    mat = ragged_matrix(301, 17, len(names), seed=5)
    want, got = tmp_path / "want.txt", tmp_path / "got.txt"
    through_id_lists(want, names, mat)
    save_walks(got, names, mat)
    assert got.read_bytes() == want.read_bytes()
    assert got.read_bytes().count(b"\n") == 301
    # the same bytes when the matrix takes several blocks, and from the int32 view a device tensor comes down as
    monkeypatch.setattr("pecanpy_amd.corpus._WRITE_ROWS", 64)
    save_walks(got, names, mat.view(np.int32))
    assert got.read_bytes() == want.read_bytes()


def test_an_empty_matrix_gives_an_empty_file(tmp_path):
    out = tmp_path / "empty.txt"
    save_walks(out, ["a", "b"], np.zeros((0, 12), dtype=np.uint32))
    assert out.read_bytes() == b""


def test_rows_of_length_zero_are_empty_lines(tmp_path):
    out = tmp_path / "blank.txt"
    save_walks(out, ["a", "b"], np.array([[1, 0, 2], [9, 9, 0], [0, 9, 1]], dtype=np.uint32))
    assert out.read_bytes() == b"b a\n\na\n"


def test_what_the_matrix_cannot_hold_is_an_error(tmp_path):
    out = tmp_path / "bad.txt"
    with pytest.raises(ValueError, match="node index 2 .*outside the 2 names"):
        save_walks(out, ["a", "b"], np.array([[1, 2, 2]], dtype=np.uint32))
    with pytest.raises(ValueError, match="row length 3 in row 1"):
        save_walks(out, ["a", "b"], np.array([[1, 0, 2], [1, 0, 3]], dtype=np.uint32))
    with pytest.raises(ValueError, match="walk matrix must be"):
        save_walks(out, ["a", "b"], np.zeros(4, dtype=np.uint32))


def test_task_walks_parses_and_the_conversion_tasks_still_convert_and_exit(tmp_path):
    a = cli.parse_args(["--input", "g.edg", "--output", "walks.txt", "--task", "walks", "--num-walks", "3", "--walk-length", "7"])
    assert (a.task, a.num_walks, a.walk_length) == ("walks", 3, 7)
    assert cli.parse_args(["--input", "g.edg", "--output", "o.emb"]).task == "pecanpy"
    with pytest.raises(SystemExit):
        cli.parse_args(["--input", "g.edg", "--output", "o", "--task", "corpus"])
    edg = tmp_path / "g.edg"
    edg.write_text("a\tb\nb\tc\n")
    for task, members in (("tocsr", {"IDs", "data", "indptr", "indices"}), ("todense", {"IDs", "data"})):
        out = str(tmp_path / f"o.{task}.npz")
        with pytest.raises(SystemExit) as stop:
            cli.read_graph(cli.parse_args(["--input", str(edg), "--output", out, "--task", task]))
        assert stop.value.code == 0 and set(np.load(out).files) == members
