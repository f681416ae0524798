"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/aerognn.h declares (no compute without a GPU), ctypes structs match the C layout,
the mirrored modules keep the reference's class names / state_dict keys / parameter counts,
and the product path refuses to run on CPU (no silent fallback)."""
import ctypes

import pytest
import torch

from golden_util import load, params


def test_library_exports_header_symbols():
    from aerognn import _lib
    lib = _lib.lib()
    names = _lib.exported_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert lib.agn_version() >= 1
    assert lib.agn_packed_bytes(128, 128, _lib.BF16) == 4 * 8 * 1024
    assert lib.agn_packed_bytes(128, 128, _lib.F32) == 2 * 4 * 8 * 1024
    assert lib.agn_error_string(-4) == b"unsupported shape"


def test_header_declares_every_exported_symbol():
    """The converse: every agn_* function in the shared object's dynamic symbol table is declared in
    include/aerognn.h (and so bound with its types)."""
    import os
    import shutil
    import subprocess
    from aerognn import _lib
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if not os.path.exists(nm):
        pytest.skip("neither nm nor llvm-nm is on this machine")
    table = subprocess.check_output([nm, "-D", "--defined-only", _lib.LIB_PATH]).decode().splitlines()
    exported = {f[2] for f in map(str.split, table) if len(f) == 3 and f[1] in "Tt" and f[2].startswith("agn_")}
    names = set(_lib.exported_symbols())
    assert len(exported) >= 20
    assert exported <= names, sorted(exported - names)


def test_struct_layouts_match_c(tmp_path):
    """The structs the reader (aerognn/_header.py) builds from include/aerognn.h agree with the C
    compiler's layout of it: the size of every struct, the offset and size of every field, pads included."""
    from abi_layout import check_struct_layouts
    from aerognn import _lib as L
    assert len(L.STRUCTS) >= 13
    for st, cls in L.STRUCTS.items():
        assert getattr(L, cls.__name__) is cls, st
    seen = check_struct_layouts(L.STRUCTS, tmp_path)
    assert seen == sum(1 + len(cls._fields_) for cls in L.STRUCTS.values())


HEADER_OK = """
#ifdef __cplusplus
extern "C" {
#endif
#define AGN_N 2
enum { AGN_A = 0, AGN_B = (-1) };
typedef struct {
  int a, b;
  const float* p[AGN_N];   /* two pointers */
  int64_t n;
} agn_t;
int agn_f(const agn_t* t, const agn_t* table_device, int64_t n,
          const void* const* pp, void* stream);
DECLARATION
const char* agn_name(void);
#ifdef __cplusplus
}
#endif
"""


def test_header_reader_reads_its_subset():
    from aerognn import _header as H
    consts, structs, protos = H.parse(HEADER_OK.replace("DECLARATION", ""))
    assert consts == {"AGN_N": 2, "AGN_A": 0, "AGN_B": -1}
    T = structs["agn_t"]
    assert T.__name__ == "T" and [f for f, _ in T._fields_] == ["a", "b", "p", "n"]
    assert (T.b.offset, T.p.offset, T.p.size, T.n.offset, ctypes.sizeof(T)) == (4, 8, 16, 24, 32)
    assert protos == {"agn_f": (ctypes.c_int, [ctypes.POINTER(T), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_void_p]),
                      "agn_name": (ctypes.c_char_p, [])}


@pytest.mark.parametrize("what,decl", [
    ("bit-field", "typedef struct { int a : 3; int b; } agn_bits;"),
    ("nested anonymous struct", "typedef struct { int a; struct { int b; } s; } agn_nested;"),
    ("unnamed parameter", "int agn_g(int, void* stream);"),
    ("unnamed pointer parameter", "int agn_g(int n, const void*);"),
    ("function-pointer parameter", "int agn_g(void (*cb)(int), void* stream);"),
    ("unknown type", "int agn_g(unsigned n, void* stream);"),
    ("pointer return", "void* agn_g(int n);"),
    ("non-integer define", "#define AGN_X 1.5"),
    ("other directive", "#include <stdio.h>"),
    ("named struct", "struct agn_s { int a; };"),
])
def test_header_reader_refuses_what_it_cannot_read(what, decl):
    """One unsupported declaration at a time: the reader raises and names the declaration's line."""
    from aerognn import _header as H
    text = HEADER_OK.replace("DECLARATION", decl)
    line = text[:text.index(decl)].count("\n") + 1
    with pytest.raises(H.HeaderError, match=rf"^hdr\.h:{line}: "):
        H.parse(text, "hdr.h")


def test_header_reader_needs_the_extern_c_block():
    from aerognn import _header as H
    with pytest.raises(H.HeaderError):
        H.parse("int agn_f(int n);")
    with pytest.raises(H.HeaderError):
        H.parse('extern "C" {\nint agn_f(int n);\n')


def test_every_bound_function_has_the_header_arity():
    """argtypes of every function reachable through lib() are set, with as many entries as the
    header's prototype has parameters (counted here from the header text, not by the reader)."""
    import re
    from aerognn import _lib
    lib = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    params = {m[1]: 0 if m[2].strip() == "void" else m[2].count(",") + 1
              for m in re.finditer(r"\b(agn_\w+)\s*\(([^()]*)\)\s*;", hdr)}
    names = _lib.exported_symbols()
    assert sorted(params) == names and len(names) >= 96
    for n in names:
        f = getattr(lib._cdll, n)
        assert f.argtypes is not None and len(f.argtypes) == params[n], n
        assert (f.restype, list(f.argtypes)) == (_lib.PROTOS[n][0], _lib.PROTOS[n][1]), n


def test_every_timed_launch_is_a_declared_function():
    """_lib.LAUNCHES (the entry points the event timer wraps) names only functions the header declares:
    a misspelt or removed one would silently go untimed."""
    from aerognn import _lib
    assert len(set(_lib.LAUNCHES)) == len(_lib.LAUNCHES)
    assert set(_lib.LAUNCHES) <= set(_lib.exported_symbols()), sorted(set(_lib.LAUNCHES) - set(_lib.exported_symbols()))


@pytest.mark.parametrize("name,ctor", [
    ("layer_sum_h32", "layer"), ("layer_cat_h32", "layer"), ("mgn5_f32", "mgn"), ("bsms_s4", "bsms"),
    ("bsms_s2_st3", "bsms")])
def test_state_dict_schema(name, ctor):
    """Reference checkpoints load unchanged; same key set and shapes."""
    d, m = load(name)
    ref = params(d)
    if ctor == "layer":
        from models.mgnLayer import MeshGraphNetLayer
        H, nh = m["H"], m["n_hid"]
        model = MeshGraphNetLayer(H, H, H, nh, nh, "relu", True, m["aggregation"], m["trick"])
    elif ctor == "mgn":
        from models.mgn import MeshGraphNet
        model = MeshGraphNet(*m["dims"], **m["kwargs"])
    else:
        from models.bsms_mgn import BiStridedMeshGraphNet
        model = BiStridedMeshGraphNet(*m["dims"], **m["kwargs"])
    sd = model.state_dict()
    assert set(sd) == set(ref)
    for k in sd:
        assert sd[k].shape == ref[k].shape, k
    model.load_state_dict(ref)


def test_same_init_as_reference():
    """Module tree + init order mirror the reference: same seed, same initial weights."""
    from models.bsms_mgn import BiStridedMeshGraphNet
    d, m = load("bsms_s4")
    torch.manual_seed(4)  # tools/make_goldens.py:case_bsms seeds 4 before building the mesh
    from aerognn.meshgen import ellipsoid  # noqa: F401  (mesh built before the model, no torch RNG)
    model = BiStridedMeshGraphNet(*m["dims"], **m["kwargs"])
    for k, v in model.state_dict().items():
        assert torch.equal(v, params(d)[k]), k


def test_param_count_c3():
    from models.bsms_mgn import BiStridedMeshGraphNet
    m = BiStridedMeshGraphNet(6, 4, 4, processor_size=15, num_hidden_layers_node_processor=2,
                              num_hidden_layers_edge_processor=2, num_hidden_layers_node_encoder=2,
                              num_hidden_layers_edge_encoder=2, num_hidden_layers_decoder=2,
                              do_concat_trick=True, num_scales=4)
    assert sum(p.numel() for p in m.parameters()) == 2877572
    assert m.__class__.__name__ == "BiStridedMeshGraphNet"    # utils.py:178-189 dispatch


def test_config_errors_match_reference():
    from models.bsms_mgn import BiStridedMeshGraphNet
    with pytest.raises(ValueError):
        BiStridedMeshGraphNet(6, 4, 4, num_scales=0)
    with pytest.raises(ValueError):
        BiStridedMeshGraphNet(6, 4, 4, stride=0)
    with pytest.raises(ValueError):
        BiStridedMeshGraphNet(6, 4, 4, num_scales=3, layers_per_scale=[1, 2, 3])


def test_cpu_tensors_fail_loudly():
    from models.mgnLayer import MeshGraphNetLayer
    layer = MeshGraphNetLayer(32, 32, 32, 2, 2, "relu", True, "add", True)
    x = torch.randn(10, 32)
    e = torch.randn(20, 32)
    ei = torch.randint(0, 10, (2, 20))
    with pytest.raises(RuntimeError):
        layer(x, e, ei)


def test_poolmgn_state_dict_and_errors():
    """poolMGN keeps the reference's module tree (state_dict keys of the golden, generated from
    /root/reference/models/poolmgn.py) and its ValueError for an unknown pooling method."""
    from golden_util import load as _load
    from models.poolmgn import poolMGN
    d, m = _load("poolmgn_mean")
    model = poolMGN(*m["dims"], **m["kwargs"])
    ref_keys = sorted(k[2:] for k in d if k.startswith("p:"))
    assert sorted(model.state_dict().keys()) == ref_keys
    model.load_state_dict(params(d))
    with pytest.raises(ValueError):
        poolMGN(6, 4, 4, global_pool_method="median")


def test_pack_rejects_float64_and_mixed_dtypes():
    """a float64 model (or a float64 weight in a 16/32-bit pack) raises on the host
    instead of being packed as float bits (agn_pack reads descriptors from device memory)."""
    import torch
    from aerognn.core import Pack
    w = torch.randn(128, 128, dtype=torch.float64)
    p = Pack()
    p.matrix("W", 128, 128, [(w, 0, 0, False)])
    with pytest.raises(NotImplementedError):
        p.update(torch.float64, torch.device("cpu"))
    with pytest.raises(TypeError):
        p.update(torch.float32, torch.device("cpu"))


def test_tile_block_counts():
    """The block-count rule the persistent tile kernels share (csrc/host.hpp tile_blocks), through
    the two exports that expose it: every CU once there is work for all, else the blocks needed
    rounded up to a multiple of 8, at least 8. The values hold for any device with >= 32 CUs
    (256 is assumed without one)."""
    from aerognn import _lib
    lib = _lib.lib()
    table = {0: (8, 8), 1: (8, 8), 17: (8, 8), 1025: (8, 16), 3072: (8, 24), 3073: (16, 32)}
    for rows, want in table.items():
        assert (lib.agn_edge_fwd32_blocks(rows), lib.agn_edge_bwd_blocks(rows)) == want, rows
    for fn in (lib.agn_edge_fwd32_blocks, lib.agn_edge_bwd_blocks):
        counts = [fn(rows) for rows in list(range(0, 4100)) + list(range(4100, 400000, 997))]
        assert all(n % 8 == 0 for n in counts)
        assert all(a <= b for a, b in zip(counts, counts[1:]))
