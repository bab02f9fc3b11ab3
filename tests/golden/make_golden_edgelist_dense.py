#!/usr/bin/env python3
"""Golden vectors for the dense classes' DEVICE edge-list reader, in the style of make_golden_edgelist_device.py: the
reference's own AdjlstGraph (src/pecanpy/graph.py:108-386) reads edge-list texts and ``to_dense()`` gives the matrix a
DenseGraph would hold.  The texts aim at what the dense build adds to the reader -- float64 weights whose float32 roundings
hide something (all 1.00000001: a unit float32 CSR; 0.1 and 0.10000000001 on two pairs: one float32), weights that ARE all
1.0, a pair repeated in another spelling, graphs of 1, 64 and 65 vertices (the tail bits of the last adjacency word), empty
rows, no trailing newline.  Inputs (the texts) and outputs (IDs, the matrix's bits, warning count or exception type) are
stored as data in tests/golden/edgelist_dense_cases.json.  Runs only where the reference tree and the stub packages of
make_golden.py are present.

usage:  python tests/golden/make_golden_edgelist_dense.py
"""
import json
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_stubs"))
sys.path.insert(1, "/root/reference/src")

import numpy as np  # noqa: E402
from pecanpy.graph import AdjlstGraph  # noqa: E402  (the reference)

SPELLINGS = ("{:.4f}", "{:.4e}", "{:g}", "+{:.5f}", "{:.4E}")   # five spellings, each exact for a multiple of 1/16 below 10


def ring_with_chords(n, chords, seed):
    """n vertices on a ring (every vertex appears, the last one included) + `chords` random pairs; the weight is a function of
    the unordered pair, spelled in one of five ways, so a repeated pair never conflicts."""
    rng = np.random.default_rng(seed)
    pairs = [(i, (i + 1) % n) for i in range(n)] + [(n - 1, 0), (0, n - 1)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, n, (chords, 2))]
    lines = []
    for a, b in pairs:
        lo, hi = min(a, b), max(a, b)
        value = ((lo * 13 + hi * 7) % 64 + 1) / 16           # a multiple of 1/16 in (0, 4]: every spelling gives the same float64
        text = SPELLINGS[(lo + hi) % len(SPELLINGS)].format(value)
        assert float(text) == value
        lines.append(f"u{a}\tu{b}\t{text}\n")
    return "".join(lines)


def cases():
    out = []

    def add(name, text, weighted, directed, delimiter="\t"):
        out.append(dict(name=name, text=text, weighted=weighted, directed=directed, delimiter=delimiter))

    # 1.00000001 rounds to 1.0f: the float32 CSR is all ones, the matrix is not
    add("all_weights_1_00000001", "a\tb\t1.00000001\nb\tc\t1.00000001\nc\ta\t1.00000001\nc\td\t1.00000001\n", True, False)
    add("all_weights_exactly_one", "a\tb\t1\nb\tc\t1.0\nc\ta\t1e0\nc\td\t1.000\nd\ta\t+1\n", True, False)
    add("one_weight_not_one", "a\tb\t1\nb\tc\t1.0\nc\ta\t1.00000001\nc\td\t1\n", True, False)
    # two DIFFERENT pairs: no conflict, one float32 value, two float64 values
    add("float32_equal_float64_distinct", "a\tb\t0.1\nc\td\t0.10000000001\nb\tc\t0.1\n", True, False)
    # the same pair again with an equal float64 in another spelling: no warning, the last insertion wins
    add("same_pair_other_spelling", "a\tb\t0.25\nb\ta\t2.5e-1\na\tc\t3\na\tb\t0.250\nc\ta\t3.0\n", True, False)
    add("same_pair_conflict", "a\tb\t0.25\nb\ta\t0.5\n", True, False)
    add("one_vertex_self_loop", "solo\tsolo\t2.5\n", True, False)
    add("one_vertex_self_loop_unweighted", "solo\tsolo\n", False, False)
    add("ring_64", ring_with_chords(64, 180, 64), True, False)
    add("ring_65", ring_with_chords(65, 200, 65), True, False)
    add("ring_65_unweighted_directed", ring_with_chords(65, 120, 66), False, True)
    # b, sink and late never start a line; late is seen first as id2; c -> sink only
    add("directed_sinks_first_seen_as_id2", "a\tb\t0.5\na\tc\t1.5\nc\tsink\t2\nd\tc\t0.75\nd\tlate\t1e-3\na\tlate\t7\n", True, True)
    add("unweighted_undirected", "x\ty\ny\tz\nz\tw\nw\tx\nx\tz\n", False, False)
    add("one_line_no_trailing_newline", "p\tq\t0.3", True, False)
    add("no_trailing_newline_directed", "p\tq\t0.3\nq\tr\t1.00000001", True, True)
    add("wrong_columns_weighted", "a\tb\t1\nb\tc\n", True, False)
    return out


def run_reference(case):
    res = dict(case)
    with tempfile.NamedTemporaryFile("w", suffix=".edg", delete=False, newline="") as f:
        f.write(case["text"])
        path = f.name
    try:
        g = AdjlstGraph()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                g.read(path, case["weighted"], case["directed"], case["delimiter"])
            except Exception as exc:  # noqa: BLE001 - the exception type is the expected output
                res["error"] = type(exc).__name__
                return res
        dense = np.asarray(g.to_dense(), dtype=np.float64)
        res.update(error="", n_warnings=len(caught), ids=list(g.nodes), num_edges=int(g.num_edges),
                   dense_bits=dense.view(np.uint64).ravel().tolist())
    finally:
        os.unlink(path)
    return res


def main():
    results = [run_reference(c) for c in cases()]
    with open(os.path.join(HERE, "edgelist_dense_cases.json"), "w") as f:
        json.dump(results, f, separators=(",", ":"))
    for r in results:
        print(f"{r['name']:36s} error={r['error'] or '-':12s} warnings={r.get('n_warnings', '-')} n={len(r.get('ids', []))}")


if __name__ == "__main__":
    main()
