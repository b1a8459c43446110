"""The C-ABI library loads on a GPU-less host and exports every symbol include/regtgcn.h declares;
host-side argument validation works without touching a GPU."""
import ctypes
import os
import re

import pytest
import torch

import regtgcn_amd as R
from regtgcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "regtgcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(regt_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = R.load_library()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/regtgcn.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes prototype in _lib.SIGNATURES"
    assert sorted(_lib.SIGNATURES) == names
    assert lib.regt_abi_version() == _lib.ABI_VERSION


def test_host_side_validation_without_gpu():
    lib = R.load_library()
    d = _lib.Dims(10, 6, 7, 256, 5, 1, 128, 1, 0.01)            # F = 7 is not a multiple of 4
    assert lib.regt_workspace_bytes(ctypes.byref(d), 1, 0) == 0
    assert b"multiple of 4" in lib.regt_last_error()
    d = _lib.Dims(104, 6, 8, 256, 5, 1, 128, 1, 0.01)
    assert lib.regt_workspace_bytes(ctypes.byref(d), 1, 0) > 104 * 6 * 256 * 4 * 9
    assert lib.regt_workspace_bytes(ctypes.byref(d), 1, 1) > lib.regt_workspace_bytes(ctypes.byref(d), 1, 0)
    rc = lib.regt_spmm_csr(None, None, None, None, None, 1, 1, 4, None)
    assert rc != 0 and b"NULL" in lib.regt_last_error()
    assert lib.regt_graph_workspace_bytes(1000, 100) > 0
    assert lib.regt_wgrad_slab_floats(1000, 256, 256, 1) >= 256 * 256 + 256


def test_developer_options_are_host_state_and_every_documented_name_is_known():
    """regt_set_option touches no GPU: every option name the header documents is accepted, returns the previous value and can be
    restored; an unknown name is refused with -1 and a message."""
    lib = R.load_library()
    src = open(os.path.join(ROOT, "include", "regtgcn.h")).read()
    doc = src[src.index("Developer switches"):src.index("int32_t regt_set_option")]
    names = sorted(set(re.findall(r'"([a-z_0-9]+)"', doc)))
    assert {"xbf", "fused_bwd", "spmm_rows", "dgrad1_gen", "tgcn_collapse", "wgrad_ring", "wgrad_tile", "wgrad_ring256", "wgrad_pairs",
            "wgrad_wave", "wgrad_bnw64"} <= set(names), names
    for n in names:
        prev = lib.regt_set_option(n.encode(), 1)
        assert prev >= 0, (n, lib.regt_last_error())
        assert lib.regt_set_option(n.encode(), prev) >= 0          # restored (the value just set is returned)
        assert lib.regt_set_option(n.encode(), prev) == prev
    assert lib.regt_set_option(b"no_such_option", 1) == -1 and b"unknown option" in lib.regt_last_error()


def test_modules_refuse_cpu_tensors_and_keep_reference_layout():
    m = R.RegionalTemporalGCN(node_features=8, num_nodes=104, periods=6, output_dim=1)
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "ref_ckpt_in6_out1_epoch50.pt"), map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(m.state_dict().keys())
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in m.state_dict().items())
    m.load_state_dict(sd, strict=True)
    with pytest.raises(R.RegtError):
        m(torch.zeros(104, 8, 6), torch.zeros(2, 0, dtype=torch.long))
    # the reference's keyword names bind like its positional parameters (models/RegionalTemporalGCN.py:25-26): a complete keyword
    # call gets as far as the device check, a wrong name is Python's TypeError
    z, e = torch.zeros(104, 8, 6), torch.zeros(2, 0, dtype=torch.long)
    kw = {f"{r}edge_index": e for r in ("IA", "KS", "KY", "OH", "WI")}
    kw.update({f"{r}edge_attr": torch.zeros(0) for r in ("IA", "KS", "KY", "OH", "WI")})
    with pytest.raises(R.RegtError):
        m(x=z, edge_index=e, **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        m(z, e, **kw, edge_weight=None)
    with pytest.raises(TypeError, match="missing 1 required"):
        m(z, e, **{k: v for k, v in kw.items() if k != "WIedge_attr"})
    t = R.TemporalGCN(node_features=8, periods=6, output_dim=3)
    assert "tgnn.linear.weight" in t.state_dict() and tuple(t.state_dict()["tgnn.linear.weight"].shape) == (256, 64)
    assert not any(k.startswith("tgnn._weight_att") for k in t.state_dict())
    import inspect
    assert list(inspect.signature(t.forward).parameters) == ["x", "edge_index", "edge_attr"]   # keyword call, run.py:188


def test_entry_points_reject_bad_arguments_before_touching_the_gpu():
    """Every model-level entry point validates dims / pointers / alignment on the host and reports through
    regt_last_error (the reference raises Python exceptions at the same places: wrong shapes, missing tensors)."""
    lib = R.load_library()
    B = ctypes.byref
    good = _lib.Dims(104, 6, 8, 256, 5, 1, 128, 1, 0.01)
    g, p, gr = _lib.Graph(), _lib.Params(), _lib.Grads()
    one = ctypes.c_void_p(256)                                    # a non-NULL, 16-byte aligned dummy that is never dereferenced

    rc = lib.regt_forward(None, B(g), B(p), one, one, one, one, 1 << 30, None)
    assert rc != 0 and b"dims is NULL" in lib.regt_last_error()
    rc = lib.regt_forward(B(good), B(g), B(p), one, one, one, one, 1 << 30, None)
    assert rc != 0 and b"graph incomplete" in lib.regt_last_error()
    g.rowptr = g.col = g.val = g.node_region = 256
    rc = lib.regt_forward(B(good), B(g), B(p), one, one, one, one, 1 << 30, None)
    assert rc != 0 and b"required tensor pointer is NULL" in lib.regt_last_error()
    bad_t = _lib.Dims(104, 256, 8, 256, 5, 1, 128, 1, 0.01)
    rc = lib.regt_forward(B(bad_t), B(g), B(p), one, one, one, one, 1 << 30, None)
    assert rc != 0 and b"exceeds 255 periods" in lib.regt_last_error()
    rc = lib.regt_cell_forward(B(good), B(g), B(p), one, one, one, one, one, 1 << 30, None)
    assert rc != 0 and b"regional must be 0" in lib.regt_last_error()
    rc = lib.regt_backward(B(good), B(g), B(p), None, one, None, one, None, one, 1 << 30, None)
    assert rc != 0                                                 # params incomplete / grads NULL
    rc = lib.regt_spmm_csr(one, one, one, one, one, 8, 8, 6, None)
    assert rc != 0 and b"multiple of 4" in lib.regt_last_error()
    rc = lib.regt_spmm_dual(one, one, one, one, one, one, one, 8, 46, None)
    assert rc != 0 and b"multiple of 4 floats" in lib.regt_last_error()
    rc = lib.regt_spmm_dual(one, one, one, one, one, one, one, 8, 2052, None)
    assert rc != 0 and b"neither a multiple of 32 floats nor at most 2048" in lib.regt_last_error()
    rc = lib.regt_linear(one, 8, 4, 8, one, 8, 4, None, 7, 0.0, one, 4, None)
    assert rc != 0 and b"act must be" in lib.regt_last_error()
    rc = lib.regt_wgrad(one, 4, one, 8, 16, 4, 8, one, 8, None, None, None)
    assert rc != 0 and b"bad argument" in lib.regt_last_error()
    assert lib.regt_set_gemm_mode(0) in (0, 1)


def test_zero_hidden_models_keep_reference_layout():
    """GraphSAGETemporalGCN / GATTemporal: state_dict keys in the order the reference's modules register them (the same
    order oracle.init_params emits, which oracle/make_goldens.py asserts against the imported reference classes)."""
    from oracle import model as M
    for name, cls in (("GraphSAGETemporalGCN", R.GraphSAGETemporalGCN), ("GATTemporal", R.GATTemporal)):
        m = cls(node_features=8, num_nodes=104, periods=6, output_dim=3)
        p = M.init_params(name, 8, 6, 3, num_nodes=104, seed=0)
        assert list(p.keys()) == list(m.state_dict().keys()), name
        assert all(tuple(p[k].shape) == tuple(v.shape) for k, v in m.state_dict().items()), name
        m.load_state_dict(p, strict=True)
        import inspect
        assert list(inspect.signature(m.forward).parameters) == ["x", "edge_index", "edge_attr"]
        with pytest.raises(R.RegtError):
            m(torch.zeros(104, 8, 6), torch.zeros(2, 0, dtype=torch.long), None)
    with pytest.raises(NotImplementedError):
        R.TGCN(8, 16, baseblock="transformer")


def test_reference_launch_line_parses():
    """The argument string of the reference's own launch script (scripts/RegionalTemporalGCN.sh:1, copied here as a string) is
    accepted by the run.py counterpart, with run.py's defaults for everything it leaves out (run.py:22-45)."""
    from regtgcn_amd import train
    line = "--num_timesteps_in 6 --num_timesteps_out 1 --tr 0.2 --model RegionalTemporalGCN --tf occrate --dataloading_type 2 --epochs 50 --decomp_type regional"
    a = train.build_parser().parse_args(line.split())
    assert (a.num_timesteps_in, a.num_timesteps_out, a.tr, a.model, a.tf, a.dataloading_type, a.epochs, a.decomp_type) == \
        (6, 1, 0.2, "RegionalTemporalGCN", "occrate", 2, 50, "regional")
    d = train.build_parser().parse_args([])
    assert (d.seed, d.lr, d.decay, d.momentum, d.bs, d.tf, d.model, d.num_timesteps_in, d.num_timesteps_out, d.checkpoint_path) == \
        (42, 1e-3, 1e-4, 0.9, 32, "available", "TemporalGCN", 8, 4, "../checkpoints/")
    for flags in ("--train_ratio 0.5 --batch_size 8 --train_feature available --edge_cut random --dataset_path ./dataset --is_preprocessed --logs",
                  "--model GraphSAGETemporalGCN", "--model GAT", "--model RandomTemporalGCN --decomp_type random",
                  "--is_pretrained --pretrained_model m.pt --pretrained_model_epoch 10"):
        train.build_parser().parse_args(flags.split())


def test_etl_target_column_follows_train_feature():
    from regtgcn_amd import etl
    assert etl.feature_columns("occrate")[-1] == 12 and etl.feature_columns("AVAILABLE")[-1] == 11
    assert etl.feature_columns("occrate")[:-1] == etl.feature_columns("available")[:-1]
    with pytest.raises(ValueError):
        etl.feature_columns("speed")


# ---- the runtime switches (csrc/options.hip): defaults, clamping, environment, one list of names ---------------------------------
# name -> (default, value stored for regt_set_option(name, v)); the next call reports the stored value as "previous"
_BOOL = lambda v: 1 if v else 0
OPTION_RULES = {
    "xbf": (1, _BOOL), "fused_bwd": (1, _BOOL), "tgcn_collapse": (1, _BOOL), "dgrad1_gen": (1, _BOOL), "spmm_rows": (0, _BOOL),
    "fused_rows": (1, lambda v: 2 if v == 2 else _BOOL(v)), "embed_kernel": (1, _BOOL),
    "wgrad_ring": (6, lambda v: 0 if v < 0 else v), "wgrad_tile": (256, lambda v: 256 if v == 256 else 128),
    "wgrad_ring256": (2, lambda v: 4 if v == 4 else 2), "wgrad_bnw64": (1, _BOOL), "wgrad_wave": (1, _BOOL),
    "wgrad_pairs": (2, lambda v: 2 if v < 0 or v > 2 else v),
}
OPTION_ENV = {"REGT_XBF": "xbf", "REGT_FUSED_BWD": "fused_bwd", "REGT_TGCN_COLLAPSE": "tgcn_collapse", "REGT_DGRAD1_GEN": "dgrad1_gen",
              "REGT_SPMM_ROWS": "spmm_rows"}
PROBES = (-1, 0, 1, 2, 3, 4, 7, 128, 256)

# runs in a fresh process (the options are process state): loads the library through regt-gcn_amd/_lib.py alone (no torch), applies
# the environment assignments of argv[3] AFTER loading, then prints what every regt_set_option call of argv[2] returned
_PROBE_SCRIPT = r"""
import importlib.util, json, os, sys
spec = importlib.util.spec_from_file_location("regt_lib", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
lib = mod.load()
os.environ.update(json.loads(sys.argv[3]))
print(json.dumps([lib.regt_set_option(n.encode(), v) for n, v in json.loads(sys.argv[2])]))
"""


def _probe(calls, env=None, late_env=None):
    import json
    import subprocess
    import sys
    clean = {k: v for k, v in os.environ.items() if not k.startswith("REGT_") or k == "REGT_LIB_DIR"}
    clean.update(env or {})
    out = subprocess.run([sys.executable, "-c", _PROBE_SCRIPT, os.path.join(ROOT, "regt-gcn_amd", "_lib.py"), json.dumps(calls),
                          json.dumps(late_env or {})], env=clean, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(got) == len(calls)
    return got


def test_option_defaults_and_clamping():
    """With no switch variable set, the first regt_set_option of every name returns its default, and every call after one that
    passed v returns the value the option's rule stores for v."""
    calls = [(n, v) for n in OPTION_RULES for v in PROBES + (0,)]
    got = iter(_probe(calls))
    for n, (dflt, rule) in OPTION_RULES.items():
        expect = dflt
        for v in PROBES + (0,):
            prev = next(got)
            assert prev == expect, (n, v, prev, expect)
            expect = rule(v)


@pytest.mark.parametrize("var,value", [("REGT_XBF", 0), ("REGT_FUSED_BWD", 0), ("REGT_TGCN_COLLAPSE", 0), ("REGT_DGRAD1_GEN", 0),
                                       ("REGT_SPMM_ROWS", 1), ("REGT_XBF", 3)])
def test_option_environment_is_read_at_first_use(var, value):
    """A switch variable of the process environment decides what the first regt_set_option of its name reports (non-zero reads as
    1) and leaves every other name at its default."""
    names = list(OPTION_RULES)
    got = _probe([(n, 1) for n in names], env={var: str(value)})
    for n, prev in zip(names, got):
        assert prev == (_BOOL(value) if n == OPTION_ENV[var] else OPTION_RULES[n][0]), (var, n, prev)


def test_option_environment_set_after_loading_still_counts():
    """The variable is read at first use, not when the library is loaded (tools/fused_trace.py sets one after importing)."""
    assert _probe([("xbf", 1), ("xbf", 1)], late_env={"REGT_XBF": "0"}) == [0, 1]


def _csrc_files():
    d = os.path.join(ROOT, "regt-gcn_amd", "csrc")
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith((".hip", ".h"))}


def _registry_rows():
    """(name | None, env | None) of every row of the option table, one row per line in csrc/options.hip."""
    src = open(os.path.join(ROOT, "regt-gcn_amd", "csrc", "options.hip")).read()
    rows = re.findall(r'^\s*\{OPT_\w+,\s*(?:"(\w+)"|nullptr),\s*(?:"(\w+)"|nullptr),', src, flags=re.M)
    assert len(rows) >= 20, rows
    return [(n or None, e or None) for n, e in rows]


def test_one_list_of_option_names():
    """The table's names are exactly what regt_set_option accepts, what include/regtgcn.h documents and what
    tests/test_gpu_switches.py holds defaults for."""
    import ast
    lib = R.load_library()
    rows = _registry_rows()
    names = {n for n, _ in rows if n}
    assert names == set(OPTION_RULES)
    for n, e in rows:
        if n:                                                # accepted: returns the previous value, which is then restored
            prev = lib.regt_set_option(n.encode(), 1)
            assert prev >= 0, (n, lib.regt_last_error())
            lib.regt_set_option(n.encode(), prev)
        elif e:                                              # environment-only: no runtime name, in either spelling
            assert lib.regt_set_option(e.encode(), 1) == -1 and lib.regt_set_option(e[5:].lower().encode(), 1) == -1
    assert {e: n for n, e in rows if n and e} == OPTION_ENV
    hdr = open(os.path.join(ROOT, "include", "regtgcn.h")).read()
    doc = hdr[hdr.index("Developer switches"):hdr.index("int32_t regt_set_option")]
    assert set(re.findall(r'"([a-z_0-9]+)"', doc)) == names
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_switches.py")).read())
    fn = next(f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == "test_every_runtime_option_is_known_and_restores")
    dicts = [a.value for a in ast.walk(fn) if isinstance(a, ast.Assign) and a.targets[0].id == "defaults"]
    defaults = ast.literal_eval(dicts[0])
    assert {k.decode(): v for k, v in defaults.items()} == {n: d for n, (d, _) in OPTION_RULES.items()}


def test_option_source_hygiene():
    """getenv lives in the registry alone, and every REGT_* word in csrc/ is a macro / enumerator of the library, a -D build switch
    or a variable the table reads: a comment cannot name a switch that no longer exists."""
    files = _csrc_files()
    assert [f for f, s in files.items() if "getenv" in s] == ["options.hip"]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "regtgcn.h")).read(), flags=re.S)
    known = set(re.findall(r"REGT_[A-Z0-9_]+", hdr))
    for s in files.values():
        known |= set(re.findall(r"^\s*#\s*define\s+(REGT_[A-Z0-9_]+)", s, flags=re.M))
    known |= {"REGT_WG_TRACE", "REGT_WG_TRACE_N", "REGT_EPI_GENERIC", "REGT_FUSED_FINE", "REGT_FUSED_ABL", "REGT_FUSED_DBG"}   # -D
    known |= {e for _, e in _registry_rows() if e}
    stale = {}
    for f, s in files.items():
        for tok in set(re.findall(r"REGT_[A-Z0-9_]+", s)):
            ok = tok in known or (tok.endswith("_") and any(k.startswith(tok) for k in known))      # "REGT_ARITH_*"
            if not ok:
                stale.setdefault(tok, []).append(f)
    assert not stale, stale
