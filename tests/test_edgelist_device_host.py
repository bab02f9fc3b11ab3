"""The text routines of the device edge-list reader (csrc/edgelist_dev.hip.h), host build (no GPU needed): the weight parser
against Python's ``float``, bit for bit, over the whole class of literals it promises to take; the line tokeniser against
``line.strip().split(delimiter)`` on every golden edge list, with the accept / decline decision of the existing host reader."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

from pecanpy_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "edgelist_cases.json")) as _f:
    CASES = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def parse(lib, text):
    """(accepted, value) of el_parse_weight on ``text``."""
    raw = text.encode("ascii")
    value = C.c_double(0.0)
    rc = lib.pw_selftest_edgelist_weight(raw, len(raw), C.byref(value))
    assert rc in (0, 1), rc
    return bool(rc), value.value


def bits(x):
    return struct.pack("<d", x)


def assert_parses_like_python(lib, literals):
    declined = [t for t in literals if not parse(lib, t)[0]]
    assert not declined, f"{len(declined)} literals of the promised class were declined, e.g. {declined[:5]}"
    wrong = [(t, parse(lib, t)[1], float(t)) for t in literals if bits(parse(lib, t)[1]) != bits(float(t))]
    assert not wrong, f"{len(wrong)} literals differ from float(), e.g. {wrong[:5]}"


def test_the_new_symbols_exist_and_are_typed(lib):
    for name in ("pw_edgelist_read_device", "pw_edgelist_ids_shape", "pw_edgelist_ids_export", "pw_edgelist_ids_destroy",
                 "pw_selftest_edgelist_weight", "pw_selftest_edgelist_line"):
        assert name in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    assert [f for f, _ in _lib.PwEdgelistDevStats._fields_] == ["upload_ms", "scan_ms", "ids_ms", "build_ms", "lines", "n_nodes",
                                                              "file_bytes"]
    assert (_lib.EDGELIST_OK, _lib.EDGELIST_NEEDS_HOST_READER, _lib.EDGELIST_IO) == (0, 1, 2)


def test_weight_forms_of_the_golden_cases(lib):
    assert_parses_like_python(lib, ["1e-3", ".5", "5.", "+2", " 3.25 ", "0.1", "0.7", "123456.789", "2", "2.0", "1.5", "2.5", "1E5",
                                    "1e+5", "007", "0.000", "\t4.5\r"])
    golden = next(c for c in CASES if c["name"] == "weights_formats")
    assert_parses_like_python(lib, [line.split("\t")[2] for line in golden["text"].splitlines()])
    random_weighted = next(c for c in CASES if c["name"] == "random_weighted")
    assert_parses_like_python(lib, sorted({line.split("\t")[2] for line in random_weighted["text"].splitlines()}))


def random_literal(rng):
    """One literal of the promised class: 1-15 significand digits behind the leading zeros, with or without a point, the power
    of ten after the point shift within [-22, 22]."""
    d = int(rng.integers(1, 16))
    digits = str(int(rng.integers(1, 10))) + "".join(str(int(x)) for x in rng.integers(0, 10, d - 1))
    zeros = "0" * int(rng.integers(0, 4)) if rng.random() < 0.3 else ""
    if rng.random() < 0.3:                      # no point
        mantissa, frac = zeros + digits, 0
    elif rng.random() < 0.2:                    # the point in front: 0.000ddd or .ddd
        lead = int(rng.integers(0, 5))
        mantissa, frac = ("0." if rng.random() < 0.5 else ".") + "0" * lead + digits, lead + d
    else:                                       # the point inside or behind the digits
        cut = int(rng.integers(1, d + 1))
        mantissa, frac = zeros + digits[:cut] + "." + digits[cut:], d - cut
    p = int(rng.integers(-22, 23))
    e = p + frac
    if e == 0 and rng.random() < 0.5:
        exponent = ""
    else:
        exponent = ("e" if rng.random() < 0.7 else "E") + ("+" if e >= 0 and rng.random() < 0.3 else "") + str(e)
    sign = "+" if rng.random() < 0.1 else "-" if rng.random() < 0.1 else ""
    return sign + mantissa + exponent


def test_ten_thousand_random_literals_equal_python_float(lib):
    rng = np.random.default_rng(20240915)
    literals = [random_literal(rng) for _ in range(10_000)]
    assert {len(t.lstrip("+-").split("e")[0].split("E")[0].replace(".", "").lstrip("0")) for t in literals} >= set(range(1, 16))
    assert any("." not in t for t in literals) and any("e-" in t for t in literals) and any("e" not in t.lower() for t in literals)
    assert_parses_like_python(lib, literals)


def test_fifteen_digit_significands_at_both_exponent_ends(lib):
    nines, odd = "999999999999999", "123456789012345"
    literals = []
    for s in (nines, odd, "100000000000001", "900719925474099"):
        literals += [s + "e22", s + "e-22", s + "E+22", s[0] + "." + s[1:] + "e36", s[0] + "." + s[1:] + "e-8", "0." + s + "e37",
                     "0." + s + "e-7", "0.000000" + s + "e-1", s + ".e22", s + ".e-22", "000" + s + "e22", "-" + s + "e22"]
    assert_parses_like_python(lib, literals)


@pytest.mark.parametrize("text", ["1234567890123456", "1.234567890123456", "0.1234567890123456", "1000000000000000", "12345678901234567890",
                                  "1e23", "1e-23", "1.5e24", "0.1e-22", "1e99999999999999999999", "1e-400",
                                  "nan", "inf", "-inf", "Infinity", "1_0", "", " ", "\t", "0x10", "0x1p3", "1e", "e5", ".", "+", "-", "1.2.3",
                                  "1 2", "1e5.0", "--1", "1d5", "٣", "1" * 70])
def test_literals_outside_the_class_decline(lib, text):
    if text.isascii():
        assert parse(lib, text)[0] is False
    else:
        raw = text.encode("utf-8")
        value = C.c_double(0.0)
        assert lib.pw_selftest_edgelist_weight(raw, len(raw), C.byref(value)) == 0


def test_non_positive_values_parse_and_are_the_callers_to_decline(lib):
    for text, want in (("0", 0.0), ("-1", -1.0), ("0.0", 0.0), ("-0", -0.0), ("0e5", 0.0)):
        ok, value = parse(lib, text)
        assert ok and bits(value) == bits(want) == bits(float(text))
    # ... which the tokeniser does: a weighted line with such a weight is declined, the same line unweighted is taken
    for w in ("0", "-1", "0.0"):
        line = f"a\tb\t{w}"
        assert tokenize(lib, line, 0, len(line), "\t", True)[0] is False
        assert tokenize(lib, line, 0, len(line), "\t", False)[0] is True


def tokenize(lib, text, lo, hi, delimiter, weighted):
    """(accepted, n_terms, first three terms, id1, id2, weight) of el_tokenize_line on the line text[lo:hi]."""
    raw = text.encode("ascii")
    n_terms, weight = C.c_uint32(0), C.c_double(0.0)
    spans = np.zeros(10, dtype=np.uint32)
    rc = lib.pw_selftest_edgelist_line(raw, lo, hi, delimiter.encode("ascii"), int(weighted), C.byref(n_terms),
                                       C.c_void_p(spans.ctypes.data), C.byref(weight))
    assert rc in (0, 1), rc
    cut = [text[int(spans[2 * k]):int(spans[2 * k]) + int(spans[2 * k + 1])] for k in range(5)]
    return bool(rc), int(n_terms.value), cut[:3], cut[3], cut[4], weight.value


def lines_of(text):
    """(lo, hi) of every line as the device reader cuts them: up to each newline, a last line without one counts."""
    out, lo = [], 0
    for i, ch in enumerate(text):
        if ch == "\n":
            out.append((lo, i))
            lo = i + 1
    if lo < len(text):
        out.append((lo, len(text)))
    return out


def bytes_are_taken(text):
    """The byte rule of el_count_kernel (and of read_edgelist): ASCII, no control bytes but \\t \\r \\n, no \\r without \\n."""
    for i, ch in enumerate(text):
        c = ord(ch)
        if c >= 0x80 or (c < 0x20 and ch not in "\t\r\n"):
            return False
        if ch == "\r" and text[i + 1:i + 2] != "\n":
            return False
    return True


def host_reader_accepts(lib, tmp_path, case):
    """The existing host reader's decision on the case (never the new reader's)."""
    path = tmp_path / (case["name"] + ".edg")
    with open(path, "w", newline="") as f:
        f.write(case["text"])
    handle = C.c_void_p()
    rc = lib.pw_edgelist_read(str(path).encode(), int(case["weighted"]), int(case["directed"]), case["delimiter"].encode(), C.byref(handle))
    if rc == 0:
        lib.pw_edgelist_destroy(handle)
    return rc == 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tokeniser_gives_pythons_terms_and_the_host_readers_decision(lib, tmp_path, case):
    text, delim, weighted = case["text"], case["delimiter"], case["weighted"]
    accepted = bytes_are_taken(text) and len(text) > 0
    seen = {}     # (id1, id2) -> float64 weight: the reference warns when a pair comes again with another value
    for lo, hi in lines_of(text):
        ok, n_terms, terms, id1, id2, weight = tokenize(lib, text, lo, hi, delim, weighted)
        want = text[lo:hi].strip().split(delim)
        assert n_terms == len(want)
        assert terms[:min(3, n_terms)] == want[:3]
        line_ok = len(want) >= 2 and (not weighted or len(want) == 3)
        if line_ok and weighted:
            try:
                value = float(want[2])
            except ValueError:
                line_ok = False
            else:
                in_class, got = parse(lib, want[2])
                line_ok = in_class and value > 0
                if in_class:
                    assert bits(got) == bits(value)
        assert ok == line_ok, (text[lo:hi], ok, line_ok)
        if not ok:
            accepted = False
            continue
        assert (id1, id2) == (want[0].strip(), want[1].strip())
        assert bits(weight) == bits(float(want[2]) if weighted else 1.0)
        for pair in ((id1, id2),) if case["directed"] else ((id1, id2), (id2, id1)):
            if seen.setdefault(pair, weight) != weight:
                accepted = False
    assert accepted == host_reader_accepts(lib, tmp_path, case)


def test_tokeniser_on_lines_python_splits_in_a_particular_way(lib):
    """Delimiters that overlap themselves, a space delimiter inside stripped text, terms beyond the third."""
    for text, delim in (("a:::b", "::"), ("a::::b", "::"), ("::a::b", "::"), ("a::b::", "::"), ("  a b  c ", " "), ("a\tb\tc\td\te", "\t"),
                        ("a,b", ",,"), ("x", "\t"), ("\t\ta\tb", "\t"), ("a \t b\r", "\t"), ("ab", "ab"), ("aXbXc", "X")):
        ok, n_terms, terms, id1, id2, _ = tokenize(lib, text, 0, len(text), delim, False)
        want = text.strip().split(delim)
        assert n_terms == len(want) and terms[:min(3, n_terms)] == want[:3], (text, delim)
        assert ok == (len(want) >= 2)
        if ok:
            assert (id1, id2) == (want[0].strip(), want[1].strip())


def test_reader_kernels_compile_for_gfx950_without_scratch_or_spills(tmp_path):
    """``hipcc --offload-arch=gfx950`` on csrc/edgelist_dev.hip.h with the library's flags: no scratch, no spills."""
    import re
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    src = tmp_path / "el_only.hip"
    src.write_text('#include "edgelist_dev.hip.h"\n')
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{csrc}",
                          "-c", str(src), "-o", str(tmp_path / "el_only.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    blocks = re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]
    kernels = ("el_count_kernel", "el_starts_kernel", "el_lines_kernel", "el_insert_kernel", "el_first_kernel", "el_number_kernel")
    figures = {}
    for b in blocks:
        name = next((k for k in kernels if k in b.split("\n")[0]), None)
        if name:
            figures[name] = {key: int(re.search(pat, b).group(1)) for key, pat in
                             (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                              ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"))}
    print(figures)
    assert sorted(figures) == sorted(kernels)
    assert all(f["scratch"] == 0 and f["vgpr_spill"] == 0 and f["sgpr_spill"] == 0 for f in figures.values()), figures
