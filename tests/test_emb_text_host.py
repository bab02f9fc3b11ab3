"""The exact ``%.6f`` formatter of the device embedding writer (csrc/emb_text.hip.h), host build (no GPU needed):
``pw_selftest_format_f6(on_device=0)`` against Python's own ``"%.6f" % float(x)``, byte for byte; and
``save_word2vec_format_device`` refuses anything but a device matrix with one name per row before the library is touched."""
import os

import numpy as np
import pytest

from emb_text_cases import adversarial_values, assert_equals_python, python_f6, selftest_f6
from pecanpy_amd import _lib, embed


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_named_cases(lib):
    """The values the formatter's contract spells out, with the strings written here (not computed)."""
    x = np.array([1 / 128, 3 / 128, -1 / 128, 0.0, -0.0, -1e-9, 0.9999995, 2.5e-7, -123456.7890625, np.inf, -np.inf, np.nan,
                  np.finfo(np.float32).max], dtype=np.float32)
    want = [b"0.007812", b"0.023438", b"-0.007812", b"0.000000", b"-0.000000", b"-0.000000", b"1.000000", b"0.000000",
            b"-123456.789062", b"inf", b"-inf", b"nan", b"340282346638528859811704183484516925440.000000"]
    assert python_f6(x) == want                                      # (the expectation itself is Python's)
    chars, lens = selftest_f6(lib, x)
    assert [bytes(c[:n]) for c, n in zip(chars, lens)] == want
    neg_nan = np.array([0xffc00000], dtype=np.uint32).view(np.float32)
    chars, lens = selftest_f6(lib, neg_nan)
    assert bytes(chars[0, :lens[0]]) == b"nan"


def test_adversarial_values_equal_python(lib):
    x = adversarial_values()
    chars, lens = selftest_f6(lib, x)
    assert_equals_python(x, chars, lens)
    assert int(lens.max()) == 47 and int(lens.min()) == 3               # -FLT_MAX ... nan


def test_random_bit_patterns_equal_python(lib):
    """2 * 10^6 float32 bit patterns drawn uniformly from all 2^32: every exponent, NaNs and denormals included."""
    rng = np.random.default_rng(20240611)
    x = rng.integers(0, 2 ** 32, size=2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    chars, lens = selftest_f6(lib, x)
    assert_equals_python(x, chars, lens)


def test_embedding_sized_values_equal_python(lib):
    """2 * 10^6 values of N(0, 0.3): the magnitudes an embedding holds."""
    rng = np.random.default_rng(20240612)
    x = (rng.standard_normal(2_000_000) * 0.3).astype(np.float32)
    chars, lens = selftest_f6(lib, x)
    assert_equals_python(x, chars, lens)


def test_save_word2vec_format_device_refuses_what_is_not_a_device_matrix(monkeypatch, tmp_path):
    torch = pytest.importorskip("torch")

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(embed._lib, "load", no_library)
    path = tmp_path / "x.emb"
    names = ["a", "b", "c", "d"]
    vec = torch.zeros((4, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="must be a CUDA tensor"):
        embed.save_word2vec_format_device(path, names, vec)                        # a CPU tensor
    with pytest.raises(ValueError, match="must be a CUDA tensor"):
        embed.save_word2vec_format_device(path, names, vec.numpy())                # not a tensor at all

    class DeviceMatrix(torch.Tensor):                      # passes for a CUDA tensor, so that the later checks are the ones
        is_cuda = True                                     # that fire: dtype, contiguity, rank, the name count

    strided = torch.zeros((4, 12), dtype=torch.float32)[:, ::2].as_subclass(DeviceMatrix)
    assert strided.is_cuda and strided.dtype == torch.float32 and tuple(strided.shape) == (4, 6) and not strided.is_contiguous()
    with pytest.raises(ValueError, match="must be contiguous"):
        embed.save_word2vec_format_device(path, names, strided)
    double = vec.to(torch.float64).as_subclass(DeviceMatrix)
    assert double.is_cuda and double.is_contiguous() and double.dtype == torch.float64
    with pytest.raises(ValueError, match="must be float32, not torch.float64"):
        embed.save_word2vec_format_device(path, names, double)
    with pytest.raises(ValueError, match=r"must be float32\[n, dim\]"):
        embed.save_word2vec_format_device(path, names, vec[0].as_subclass(DeviceMatrix))     # one dimension

    d_vec = vec.as_subclass(DeviceMatrix)
    with pytest.raises(ValueError, match="3 node names for 4 rows"):
        embed.save_word2vec_format_device(path, names[:3], d_vec)
    with pytest.raises(ValueError, match="5 node names for 4 rows"):
        embed.save_word2vec_format_device(path, np.array(names + ["e"]), d_vec)
    assert not path.exists()


def test_embed_to_file_decides_its_route_once_where_the_walks_leave_the_device(monkeypatch, tmp_path):
    """Where ``_train_on_device`` returns ``None`` (``torch.distributed``, the multi-GPU engine) ``embed_to_file`` goes on as
    ``embed_array`` does from there -- host walk matrix, ``train_sgns``, the host writer -- without asking a second time."""
    from pecanpy_amd import pecanpy as node2vec

    k = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "karate_csr.npz"))
    g = node2vec.SparseOTF.from_csr(k["indptr"], k["indices"], k["data"], node_ids=list(k["ids"]), p=1, q=0.5, random_state=0)
    asked = []
    mat = np.arange(12, dtype=np.uint32).reshape(3, 4)
    vec = (np.random.default_rng(3).standard_normal((g.num_nodes, 5)) * 0.3).astype(np.float32)
    monkeypatch.setattr(g, "_train_on_device", lambda *a: asked.append(a))             # returns None
    monkeypatch.setattr(g, "simulate_walks_array", lambda num_walks, walk_length: mat)
    monkeypatch.setattr(g, "_device_index", lambda: 0)
    monkeypatch.setattr(embed, "train_sgns", lambda m, n, **kw: vec if m is mat and n == g.num_nodes else None)
    got, want = tmp_path / "got.emb", tmp_path / "want.emb"
    g.embed_to_file(got, dim=5, num_walks=2, walk_length=3, workers=1)
    assert len(asked) == 1
    embed.save_word2vec_format(want, g.nodes, vec)
    assert got.read_bytes() == want.read_bytes()
    st = g.last_embed_stats
    assert st["vectors_host_bytes"] == vec.nbytes and st["walk_matrix_host_bytes"] == 2 * mat.nbytes
    assert {"walk_ms", "sgns_call_ms", "write_call_ms"} <= set(st)
    assert g.embed_array(dim=5, num_walks=2, walk_length=3, workers=1) is vec and len(asked) == 2
    assert sorted(g.last_embed_stats) == ["sgns_call_ms", "walk_matrix_host_bytes", "walk_ms"]  # embed_array's record is its own


def test_writer_kernels_compile_for_gfx950_without_scratch_or_spills(tmp_path):
    """``hipcc --offload-arch=gfx950`` on csrc/emb_text.hip.h with the library's flags: the compiler's resource remarks must
    show no scratch and no spills (the decomposition's five limbs stay in registers: every index into them is static).

    The scan of the row counts is csrc/scan.hip.h's kernel pair in the 64-bit in-place instantiation the writers launch.

    Figures of this tree: VGPRs 46 (f6_selftest_kernel) / 58 (emb_count_kernel) / 38 and 48 (the scan) / 74
    (emb_fill_kernel, 12 416 bytes of LDS), scratch 0 bytes per lane and no spills in all five."""
    import os
    import re
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(os.path.dirname(os.path.abspath(embed.__file__)), "csrc")
    src = tmp_path / "emb_only.hip"
    src.write_text('#include "emb_text.hip.h"\n'
                   'template void pw::exclusive_scan_inplace<uint64_t>(hipStream_t, uint64_t *, uint64_t, uint64_t *);\n')
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{csrc}",
                          "-c", str(src), "-o", str(tmp_path / "emb_only.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    blocks = re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]
    kernels = ("f6_selftest_kernel", "emb_count_kernel", "tile_sums_kernel", "tile_offsets_kernel", "emb_fill_kernel")
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
