"""Records what the conv wrappers of srganst.ops hand to the launch seam (ops._launch) -> tests/golden/launch_routes.json.

The wrappers run without a GPU: tensors live on the `meta` device, ops.ptr / ops._dptr / ops.check are stubs and ops._launch is a
recorder, so the only code that runs is the routing in ops.py and the library's host-side queries.  Per call the table keeps the
launch (label, entry symbol, trace name, FLOPs, the argument tuple with pointers reduced to null / non-null, the shapes of the
keep-alive tensors), the shapes of what the wrapper returns, and a refusal as the exception's type.  Record it from a checkout of the
commit whose behaviour is to be preserved, with that checkout's own build of the library:

    python tests/golden/make_golden_launch_routes.py

tests/test_launch_routes.py replays the table against the tree under test; no cell is ever re-recorded from that tree.
"""
import contextlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "srgan-st_amd"))
OUT = os.path.join(HERE, "launch_routes.json")

_spec = importlib.util.spec_from_file_location("make_golden_selection", os.path.join(HERE, "make_golden_selection.py"))
mgs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgs)

# switches the table is repeated under, one at a time ("" = none): an environment variable, or an attribute of srganst.ops
SWITCHES = ["", "SST_CONV_PIPE=0", "CONV_NS=False", "S2D_EPI=True", "S2D_EPI_GRP=True", "TRACE={}"]


def shapes():
    """The 3x3 rows of the selection table's grid."""
    return [r for r in mgs.shapes() if r[5] == 3]


@contextlib.contextmanager
def switched(ops, sw):
    """Sets `sw` alone (every other SST_* variable unset), restores environment and attributes on exit."""
    from srganst import _abi
    env = dict(os.environ)
    attrs = {k: getattr(ops, k) for k in ("CONV_NS", "S2D_EPI", "S2D_EPI_GRP", "TRACE")}
    try:
        for k in [k for k in os.environ if k.startswith("SST_") and k != "SST_LIB_PATH"]:
            del os.environ[k]
        ops.CONV_NS, ops.S2D_EPI, ops.S2D_EPI_GRP, ops.TRACE = True, False, False, None
        if sw.startswith("SST_"):
            os.environ.__setitem__(*sw.split("="))
        elif sw:
            k, v = sw.split("=")
            setattr(ops, k, {"True": True, "False": False, "{}": {}}[v])
        _abi.reload_env()
        yield
    finally:
        os.environ.clear()
        os.environ.update(env)
        for k, v in attrs.items():
            setattr(ops, k, v)
        _abi.reload_env()


@contextlib.contextmanager
def stubbed(ops, launches):
    """ops without a device: pointers become "p" (None stays None), nothing is checked, every launch is appended to `launches`."""
    import torch
    saved = {k: getattr(ops, k) for k in ("ptr", "_dptr", "check", "_launch")}

    def shp(keep):
        return sorted(list(t.shape) for t in keep if torch.is_tensor(t))

    def launch(fn, args, what, flops, name_fn, keep):
        launches.append([what, fn.__name__, name_fn(), flops, [0 if a is None else a for a in args], shp(keep)])
    try:
        ops.ptr = ops._dptr = lambda t: None if t is None else "p"
        ops.check = lambda rc, what=None: None
        ops._launch = launch
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def calls(ops, row):
    """(case name, thunk) for one shape row; the thunk returns (wrapper's return value, extra)."""
    import torch
    from srganst import _abi
    B, H, W, cin, cout, k, s = row
    L = _abi.lib()
    t = lambda *shape: torch.empty(*shape, device="meta", dtype=torch.float32)
    ho, wo = ops.conv_out_hw(H, W, k, s)
    grp = B // 2
    coef = lambda c: t(B // grp, c) if grp else t(c)
    x, wp = t(B, H, W, cin), t(L.sst_conv_packed_floats(cout, cin, k))
    fwd = lambda **kw: (lambda: (ops.conv_fwd(x, wp, cout, k, s, bias=t(cout), **kw), None))
    out = [("fwd", fwd()), ("fwd_stats", fwd(want_stats=True)), ("fwd_res", fwd(residual=t(B, ho, wo, cout))), ("fwd_pre", fwd(want_pre=True))]
    if cout % 4 == 0:
        out += [("fwd_shuffle", fwd(out_mode=ops.OUT_SHUFFLE)), ("fwd_shuffle_stats", fwd(out_mode=ops.OUT_SHUFFLE, want_stats=True))]
    out.append(("fwd_grp", fwd(grp=grp, in_scale=coef(cin), in_shift=coef(cin), in_slope_const=0.2, in_act=ops.ACT_SLOPE)))
    if s == 1:
        epi = lambda c=t: dict(epi_scale=c(cout), epi_shift=c(cout), epi_slope_const=0.2, epi_act=1)
        dg = lambda **kw: (lambda: (ops.conv_dgrad_bwdstats(x, wp, cout, k, t(B, H, W, cout), **kw), None))
        out += [("dgrad_res", dg(residual=t(B, H, W, cout), **epi())), ("dgrad", dg(**epi())), ("dgrad_grp", dg(grp=grp, **epi(coef)))]
    else:
        dy, wd = t(B, ho, wo, cout), t(L.sst_conv_s2_dgrad_packed_floats(cout, cin))
        for g in (0, grp):
            c = coef if g else t
            e = dict(y=t(B, H, W, cin), scale=c(cin), shift=c(cin), slope=None, slope_const=0.2, act=1)
            out += [(f"s2_g{int(bool(g))}", lambda g=g: (ops.conv_s2_dgrad(dy, wd, H, W, cin, grp=g), None)),
                    (f"s2_epi_g{int(bool(g))}", lambda g=g, e=e: (ops.conv_s2_dgrad(dy, wd, H, W, cin, epi=e, grp=g), None))]

    def wgrad(defer):
        r = ops.conv_wgrad(x, t(B, ho, wo, cout), t(cout, cin, k, k), k, s, defer_reduce=defer)
        return r, defer
    out += [("wgrad", lambda: wgrad(None)), ("wgrad_defer", lambda: wgrad([]))]
    return out


def _plain(v):
    """Tensors -> their shapes, through tuples / lists; None and numbers as they are."""
    import torch
    if torch.is_tensor(v):
        return list(v.shape)
    if isinstance(v, (tuple, list)):
        return [_plain(e) for e in v]
    return v


def record(ops, shape_rows):
    """One row per shape: {case: record}, in the form json.loads gives back (tuples as lists)."""
    table = []
    for row in shape_rows:
        cells = {}
        for name, thunk in calls(ops, row):
            launches = []
            with stubbed(ops, launches):
                try:
                    ret, extra = thunk()
                    rec = {"launches": launches, "ret": _plain(ret), "extra": _plain(extra)}
                except Exception as e:              # a refusal: its type is the record
                    rec = {"raises": type(e).__name__}
            cells[name] = json.loads(json.dumps(rec))
        table.append(cells)
    return table


def tables(ops, shape_rows):
    out = {}
    for sw in SWITCHES:
        with switched(ops, sw):
            out[sw] = record(ops, shape_rows)
    return out


# --- the stored form.  A record is kept as [template, literal, ...]: the template is the record with every integer >= 4 replaced by
# the name of a shape quantity it equals ("=H", "=co", ...; the FLOPs by "=F") or, failing that, by "$i" = the cell's i-th literal
# (statistics rows, workspace and slab sizes), and every list of three or more items by "#j" = parts[j].  Templates and parts are
# shared between shapes, which is what keeps the file small; decoding is exact whichever name a number happened to get.
def _symbols(row):
    B, H, W, cin, cout, k, s = row
    ho, wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    return {"B": B, "H": H, "W": W, "ci": cin, "co": cout, "ho": ho, "wo": wo, "2ho": 2 * ho, "2wo": 2 * wo, "co/4": cout // 4,
            "F": 2.0 * B * ho * wo * cout * cin * k * k}


def _big(v):
    return isinstance(v, int) and not isinstance(v, bool) and v >= 4


def _encode(v, sym, lits, parts, sigs):
    """parts: the pool (list); sigs: signature (the list with its big integers blanked) -> indices of the parts that have it."""
    if isinstance(v, dict):
        return {k: _encode(e, sym, lits, parts, sigs) for k, e in v.items()}
    if isinstance(v, float) and v == sym["F"]:
        return "=F"
    if _big(v):
        name = next((n for n, val in sym.items() if n != "F" and val == v), None)
        if name is None and v not in lits:
            lits.append(v)
        return "=" + name if name else f"${lits.index(v)}"
    if not isinstance(v, list):
        return v
    v = [e if _big(e) else _encode(e, sym, lits, parts, sigs) for e in v]
    if len(v) < 3:
        return [_encode(e, sym, lits, parts, sigs) for e in v]
    sig = json.dumps(["?" if _big(e) else e for e in v])
    for j in sigs.get(sig, ()):                 # an existing part that decodes to v (possibly through literals this cell has not used yet)
        trial = list(lits)
        for tok, e in zip(parts[j], v):
            if _big(e):
                if tok[0] == "$" and int(tok[1:]) == len(trial):
                    trial.append(e)
                if (sym[tok[1:]] if tok[0] == "=" else trial[int(tok[1:])] if int(tok[1:]) < len(trial) else None) != e:
                    break
        else:
            lits[:] = trial
            return f"#{j}"
    parts.append([_encode(e, sym, lits, parts, sigs) for e in v])
    sigs.setdefault(sig, []).append(len(parts) - 1)
    return f"#{len(parts) - 1}"


def _decode(v, sym, lits, parts):
    if isinstance(v, str) and v[:1] == "#":
        v = parts[int(v[1:])]
    if isinstance(v, list):
        return [_decode(e, sym, lits, parts) for e in v]
    if isinstance(v, dict):
        return {k: _decode(e, sym, lits, parts) for k, e in v.items()}
    if isinstance(v, str) and v[:1] == "=":
        return sym[v[1:]]
    if isinstance(v, str) and v[:1] == "$":
        return lits[int(v[1:])]
    return v


def expand(doc):
    """switch -> one {case: record} per shape.  Per switch the file keeps only the cells that differ from the table without one."""
    tpl = doc["templates"]
    cell = lambda c, row: _decode(tpl[c[0]], _symbols(row), c[1:], doc["parts"])
    named = lambda cells: {doc["cases"][int(j)]: c for j, c in (enumerate(cells) if isinstance(cells, list) else cells.items()) if c is not None}
    base = [{n: cell(c, row) for n, c in named(cells).items()} for row, cells in zip(doc["shapes"], doc["base"])]
    full = {"": base}
    for sw, diff in doc["switches"].items():
        full[sw] = [dict(b, **{n: cell(c, row) for n, c in named(diff.get(str(i), {})).items()})
                    for i, (row, b) in enumerate(zip(doc["shapes"], base))]
    return full


def main():
    from srganst import ops
    shape_rows, pool, parts, sigs, cases = shapes(), {}, [], {}, []
    t = tables(ops, shape_rows)

    def cell(rec, row):
        lits = []
        txt = json.dumps(_encode(rec, _symbols(row), lits, parts, sigs), separators=(",", ":"))
        return [pool.setdefault(txt, len(pool))] + lits
    for cells in t[""]:
        cases += [n for n in cells if n not in cases]
    enc = {sw: [{n: cell(r, row) for n, r in cells.items()} for row, cells in zip(shape_rows, t[sw])] for sw in SWITCHES}
    diff = lambda sw: {str(i): {str(cases.index(n)): c for n, c in r.items() if t[sw][i][n] != t[""][i][n]}
                       for i, r in enumerate(enc[sw]) if t[sw][i] != t[""][i]}
    doc = {"shapes": shape_rows, "cases": cases, "parts": parts, "templates": [json.loads(s) for s in pool],
           "base": [[r.get(n) for n in cases] for r in enc[""]], "switches": {sw: diff(sw) for sw in SWITCHES[1:]}}
    assert expand(json.loads(json.dumps(doc))) == t
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": ' + mgs._dump(v) for k, v in doc.items()) + "\n}\n")
    print(f"{OUT}: {len(shape_rows)} shapes, {len(pool)} templates, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
