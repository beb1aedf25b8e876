"""CPU: the C-ABI library loads, exports every symbol include/jmac_hip.h declares, validates arguments
before touching a device, and the product path refuses to run without a HIP device (no CPU fallback)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import jmac_amd
from jmac_amd import _lib


def test_library_exports_every_declared_symbol():
    names = _lib.header_symbols()
    assert len(names) >= 25
    L = _lib.lib()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert set(_lib._SIGS) == set(names)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported


def _c_kind(decl: str) -> str:
    """Kind of a C type as the header spells it: any pointer (jmac_stream_t is void*) or the scalar it names."""
    if "*" in decl or decl == "jmac_stream_t":
        return "pointer"
    scalar = {"int64_t": "int64", "int32_t": "int32", "int": "int32", "float": "float", "double": "double",
              "size_t": "size_t", "void": "void"}
    return scalar[" ".join(w for w in decl.split() if w != "const")]


def _ctypes_kind(t) -> str:
    """Kind of a ctypes type in _lib's tables (None = void return)."""
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    scalar = {ctypes.c_int64: "int64", ctypes.c_int32: "int32", ctypes.c_float: "float", ctypes.c_double: "double",
              ctypes.c_size_t: "size_t"}
    return scalar[t]


def _prototypes(path):
    """name -> (return type, [parameter types]) of every function the header declares."""
    text = "\n".join(l for l in _lib.header_text(path).splitlines() if not l.lstrip().startswith("#"))
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s*]*?)\b(jmac_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(m.group(3).split())
        types = []
        for p in ([] if params in ("", "void") else params.split(",")):
            t = re.sub(r"\s*\b[A-Za-z_]\w*$", "", p.strip())       # drop the parameter's name
            assert t, (m.group(2), p)
            types.append(t)
        out[m.group(2)] = (" ".join(m.group(1).split()), types)
    return out


@pytest.mark.parametrize("header,sigs", [("jmac_hip.h", _lib._SIGS), ("jmac_hip_testing.h", _lib._TESTING_SIGS)])
def test_ctypes_signatures_match_the_header(header, sigs):
    """Every ctypes signature in _lib has the header prototype's argument count, and per position and for the return value
    the same kind of type: a wrong int32 / int64 / float would otherwise pass garbage to a kernel without any error."""
    path = os.path.join(os.path.dirname(_lib.HEADER_PATH), header)
    protos = _prototypes(path)
    assert sorted(protos) == _lib.header_symbols(path)                # every declared function was parsed
    assert set(sigs) == set(protos)
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        res, args = sigs[name]
        if _ctypes_kind(res) != _c_kind(ret):
            bad.append("%s: returns %s, ctypes says %s" % (name, ret, res))
        if len(args) != len(params):
            bad.append("%s: %d arguments, ctypes says %d" % (name, len(params), len(args)))
            continue
        for i, (p, a) in enumerate(zip(params, args)):
            if _ctypes_kind(a) != _c_kind(p):
                bad.append("%s: argument %d is %s, ctypes says %s" % (name, i, p, a.__name__))
    assert not bad, "\n".join(bad)


def test_argument_validation_needs_no_device():
    L = _lib.lib()
    assert L.jmac_version() >= 100
    assert L.jmac_l1_score_f32(None, 4, None, 4, -1, 3, 4, None, 4, 0, None) == -1          # negative size
    assert L.jmac_l1_score_f32(None, 4, None, 4, 2, 3, 4, None, 4, 0, None) == -1           # null pointers
    assert L.jmac_sim_matrix_f32(ctypes.c_void_p(16), 3, ctypes.c_void_p(16), 4, 2, 2, 4, ctypes.c_void_p(16), 2, None) == -2
    assert L.jmac_csr_build(None, None, -5, 3, 2, None, None, None, None, None, 0, None) == -1
    assert b"workspace" in L.jmac_strerror(-3)
    assert L.jmac_items_max(10, 100, 8, 0) == 10 + 12 + 1
    assert L.jmac_items_max(10, 100, 8, 8) == 10 + 12 + 1 + 3 * 11           # cooperative splits: 3 extra items each
    assert L.jmac_rel_attn_fwd_workspace_bytes(4, 300) >= 4 * 300 * 4 + 32


def test_no_cpu_fallback():
    from jmac_amd.layer import RelationAwareLayer
    from util import make_args
    layer = RelationAwareLayer(8, 8, 8, act=torch.tanh, args=make_args())
    x, r = torch.randn(5, 8), torch.randn(3, 8)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(_lib.JmacError):
        layer(x, r, ei, torch.tensor([0, 1]))
    from jmac_amd import scoring
    with pytest.raises(_lib.JmacError):
        scoring.l1_scores(torch.randn(2, 8), torch.randn(3, 8))


def test_product_never_imports_oracle():
    root = os.path.dirname(os.path.abspath(jmac_amd.__file__))
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dp, f)).read()
                assert "oracle" not in text.replace("# oracle", ""), os.path.join(dp, f)


def test_native_sources_read_no_environment():
    """What a launcher picks depends on its arguments alone: no source of the library reads the process environment.  (A
    source scan: the library's undefined symbols list getenv whatever the project's code does, through the rocprim headers.)
    Nor does a build flag: the only preprocessor conditionals are a header's include guard (#ifndef X directly followed by
    #define X) and the testing library's JMAC_TESTING_BUILD."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(jmac_amd.__file__)), "csrc")
    srcs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    assert len(srcs) >= 10 and "aggregate.hip" in srcs
    assert [f for f in srcs if "getenv" in open(os.path.join(csrc, f)).read()] == []
    cond = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
    found = []
    for f in srcs:
        lines = open(os.path.join(csrc, f)).read().split("\n")
        for i, line in enumerate(lines):
            m = cond.match(line)
            if not m:
                continue
            rest = m.group(2).split("//")[0].strip()
            if rest in ("JMAC_TESTING_BUILD", "defined(JMAC_TESTING_BUILD)", "!defined(JMAC_TESTING_BUILD)"):
                continue
            guard = f.endswith(".h") and m.group(1) == "ifndef" and i + 1 < len(lines) and re.match(r"^\s*#\s*define\s+%s\s*$" % re.escape(rest), lines[i + 1])
            if not guard:
                found.append("%s:%d: %s" % (f, i + 1, line.strip()))
    assert found == []


def test_state_dict_keys_match_reference():
    from util import load_golden, make_args
    from jmac_amd.model import JMAC
    g = load_golden("model_small")
    ref_keys = sorted(k[len("state."):] for k in g if k.startswith("state."))
    args = make_args(dim=int(g["d"]), dropout=0.0, num_gcn_layer=2, num_negative=5, margin_align=1.0,
                     margin_completion=5.0, batch_size=40, no_name_info=False, device="cpu")
    m = JMAC(args, g["name_emb"], 2 * int(g["nrel"]), int(g["n1"]) + int(g["n2"]))
    assert sorted(m.state_dict().keys()) == ref_keys
    m.load_state_dict({k: torch.from_numpy(g["state." + k]) for k in ref_keys}, strict=True)


def test_bench_refuses_to_run_without_a_gpu():
    """bench.py measures the product path only: on a box without a HIP device it exits with a message instead of
    timing a CPU stand-in (the cpu_baseline leg is the only place the oracle is timed, beside a GPU run)."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode != 0 and "MI355X" in (res.stderr + res.stdout) and res.stdout.strip() == ""


def _bench(*args, env=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(root, "bench.py")] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, env=e, timeout=300)


def test_bench_gpus_flag_spawns_that_many_ranks():
    """`python bench.py --gpus N` with no launcher around it starts N ranks itself (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set, one rendezvous address shared by all) -- the dry launch stops each rank before it touches a GPU."""
    import json
    res = _bench("--gpus", "2", "--dry-launch")
    assert res.returncode == 0, res.stderr
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert sorted(l["rank"] for l in lines) == [0, 1]
    assert all(l["world"] == 2 and l["local_rank"] == l["rank"] for l in lines)
    assert len({l["master"] for l in lines}) == 1 and lines[0]["master"].startswith("127.0.0.1:")


def test_bench_fails_when_a_rank_fails_or_the_world_disagrees():
    # a launcher that started a different number of ranks than --gpus says: refuse instead of reporting n_gpus wrongly
    res = _bench("--gpus", "4", "--dry-launch", env={"WORLD_SIZE": "2", "RANK": "0"})
    assert res.returncode != 0 and "WORLD_SIZE" in res.stderr
    # no HIP device here: every child exits non-zero, and so must the parent
    res = _bench("--gpus", "2", "--steps", "1")
    assert res.returncode != 0


def test_index_range_check_on_host_data():
    """Out-of-range ids raise IndexError like torch indexing in the reference (host data is checked on the host)."""
    import numpy as np
    _lib.check_index_range([0, 3, 2], 4)
    _lib.check_index_range(np.array([], dtype=np.int64), 0)
    _lib.check_index_range(torch.tensor([1, 2]), 3)
    with pytest.raises(IndexError):
        _lib.check_index_range([0, 4], 4, "edge_type")
    with pytest.raises(IndexError):
        _lib.check_index_range(torch.tensor([-1, 2]), 3)
    from jmac_amd.model import _idx
    with pytest.raises(IndexError):
        _idx(np.array([5.0, 1.0]), "cpu", 5)
    assert getattr(_idx([1, 2], "cpu", 5), "_jmac_range_ok") == 5
