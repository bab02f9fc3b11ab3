#!/usr/bin/env python3
"""Golden vectors for the DEVICE edge-list reader, in the style of make_golden_edgelist.py: the reference's own AdjlstGraph
(src/pecanpy/graph.py:108-386) is run on edge-list texts that aim at what the device reader adds -- float64 weights that
conflict although their float32 roundings agree, literals outside the class it parses exactly, long ids, one slot of the id
table under contention; inputs (the texts) and outputs (IDs, CSR, num_edges, warning count or exception type) are stored as
data in tests/golden/edgelist_device_cases.json.  Runs only where the reference tree and the stub packages of make_golden.py
are present.

usage:  python tests/golden/make_golden_edgelist_device.py
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


def cases():
    out = []

    def add(name, text, weighted, directed, delimiter="\t"):
        out.append(dict(name=name, text=text, weighted=weighted, directed=directed, delimiter=delimiter))

    # the two literals differ in float64 and round to the same float32: the reference compares Python floats and warns
    add("float64_conflict_same_float32", "a\tb\t0.1\nb\ta\t0.10000000001\n", True, False)
    add("float64_equal_other_spelling", "a\tb\t0.1\nb\ta\t1e-1\na\tb\t0.10\n", True, False)
    add("sixteen_digit_weight", "a\tb\t0.1234567890123456\nb\tc\t2\n", True, False)
    add("exponent_beyond_22", "a\tb\t1e23\nb\tc\t1e-23\n", True, True)
    add("fifteen_digits_at_the_ends", "a\tb\t999999999999999e22\nb\tc\t123456789012345e-22\nc\td\t9.99999999999999e-8\n", True, True)
    long_id = "L" + "0123456789" * 30 + "x"          # 302 bytes: longer than one lane's 16 bytes many times over
    assert len(long_id) >= 300
    add("long_id", f"a\t{long_id}\n{long_id}\tb\t\nshort\t{long_id[:-1]}\n{long_id}\ta\n", False, False)
    add("hub_on_every_line", "".join(f"hub\tv{i % 37}\n" if i % 3 else f"v{i % 41}\thub\n" for i in range(300)), False, False)
    add("hub_directed_weighted", "".join(f"hub\tv{i % 29}\t{1 + (i % 29) / 4}\n" for i in range(200)), True, True)
    add("first_seen_as_id2_late", "a\tb\nb\tc\na\tc\nc\tlate\nlate\ta\n", False, True)
    add("directed_with_sinks", "a\tb\na\tc\nd\tc\nd\tsink\n", False, True)
    add("one_line", "only\tedge\n", False, False)
    add("one_line_no_newline_weighted", "p\tq\t2.5", True, False)
    add("empty_file", "", False, False)
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
        indptr, indices, data = g.to_csr()
        res.update(error="", n_warnings=len(caught), ids=list(g.nodes), num_edges=int(g.num_edges),
                   indptr=np.asarray(indptr).tolist(), indices=np.asarray(indices).tolist(),
                   data_bits=np.asarray(data, dtype=np.float32).view(np.uint32).tolist())
    finally:
        os.unlink(path)
    return res


def main():
    results = [run_reference(c) for c in cases()]
    with open(os.path.join(HERE, "edgelist_device_cases.json"), "w") as f:
        json.dump(results, f, separators=(",", ":"))
    for r in results:
        print(f"{r['name']:32s} error={r['error'] or '-':12s} warnings={r.get('n_warnings', '-')}")


if __name__ == "__main__":
    main()
