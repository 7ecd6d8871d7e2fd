"""Records what the library's host-side kernel selectors answer for a grid of conv shapes -> tests/golden/selection.json.

The selectors (kernel names, slab chunk counts, pending reduces, tile counts) are pure host code, so this runs without a GPU.
Record the table from a library built from the commit whose behaviour is to be preserved:

    SST_LIB_PATH=/path/to/that/libsrganst.so python tests/golden/make_golden_selection.py

and, with the library under test, mark the names that changed because the recorded one disagreed with the recording library's own
launcher (the numbers are never re-recorded: any difference there is an error):

    python tests/golden/make_golden_selection.py --mark-corrected

tests/test_selection_table.py replays the table against the built library.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "srgan-st_amd"))
OUT = os.path.join(HERE, "selection.json")

# dev switches the table is repeated under, one at a time ("" = none set)
SWITCHES = ["", "SST_WGRAD_S2=0", "SST_WGRAD_S1T=1", "SST_WGRAD_BAND=0", "SST_WGRAD_BAND=1", "SST_WGRAD_NO_K3C3=1",
            "SST_WGRAD_NO_K3C3_MFMA=1", "SST_WGRAD_TILE_NO_DIRECT=1", "SST_NO_TO3=1", "SST_NO_C3IN=1", "SST_NO_C3IN_MFMA=1",
            "SST_S2DGRAD4=0"]

# columns of a row; the *name* columns hold indices into "names"
FIELDS = (["wgrad_name", "chunks2_n1", "chunks2_n2", "chunks2_n16", "pending_s0a0", "pending_s0a1", "pending_s1a0", "pending_s1a1",
           "groups_ok"] + [f"conv_name_m{m}f{f}" for m in range(4) for f in range(2)] +
          ["stat_tiles", "s2_dgrad_name_f0", "s2_dgrad_name_f1", "s2_dgrad_tiles"])
NAME_COLS = [i for i, f in enumerate(FIELDS) if "name" in f]


def shapes():
    """(B, H, W, Cin, Cout, ksize, stride) rows: the layers of both networks, then the edge shapes of the GPU tests."""
    rows = []
    for crop in (96, 192):
        lr = crop // 4
        layers = [(lr, 3, 64, 9, 1), (lr, 64, 64, 3, 1), (lr, 64, 256, 3, 1), (lr, 256, 64, 3, 1), (2 * lr, 64, 256, 3, 1),
                  (2 * lr, 256, 64, 3, 1), (crop, 64, 3, 9, 1)]                                        # generator (+ data-gradient roles)
        c = 64
        for i, hw in enumerate((crop, crop // 2, crop // 4, crop // 8)):                              # discriminator
            cin = 3 if i == 0 else c
            cout = 64 if i == 0 else 2 * c
            layers += [(hw, cin, cout, 3, 1), (hw, cout, cin, 3, 1), (hw, cout, cout, 3, 2)]
            c = cout
        for B in (1, 2, 16, 32):
            rows += [(B, hw, hw, cin, cout, k, s) for hw, cin, cout, k, s in layers]
    k3 = lambda cases, s=None: [(c[0], c[1], c[2], c[3], c[4], 3, s if s is not None else c[5]) for c in cases]
    # test_conv_wgrad_all_taps_tile_kernel
    rows += k3([(3, 32, 48, 64, 64, 2), (2, 24, 24, 128, 96, 2), (5, 12, 12, 96, 160, 2), (16, 12, 12, 512, 512, 2), (1, 4, 16, 32, 32, 2),
                (2, 96, 96, 64, 64, 2), (2, 8, 16, 32, 32, 1), (3, 16, 24, 64, 96, 1), (2, 12, 12, 64, 32, 1), (16, 12, 12, 256, 512, 1),
                (1, 4, 8, 32, 64, 1), (2, 48, 48, 64, 128, 1)])
    # test_conv_wgrad_3_channel_input_mfma_kernel / test_conv_fwd_three_channel_input_mfma_kernel
    rows += k3([(2, 8, 32, 3, 64), (3, 5, 64, 3, 64), (1, 1, 32, 3, 64), (2, 12, 96, 3, 64), (1, 7, 192, 3, 64)], 1)
    # test_conv_wgrad_band_kernel
    rows += k3([(2, 24, 24, 64, 64), (1, 48, 48, 64, 128), (3, 12, 12, 128, 64), (1, 9, 16, 64, 64), (2, 6, 8, 64, 64), (16, 24, 24, 64, 64)], 1)
    # three-channel input (VALU forms) and the 64 -> 3 kernel
    rows += k3([(2, 24, 20, 3, 64), (3, 13, 9, 3, 128), (2, 8, 8, 3, 16), (2, 13, 9, 3, 64), (2, 8, 8, 3, 6)], 1)
    rows += k3([(2, 8, 32, 64, 3), (3, 5, 20, 64, 3), (1, 7, 192, 64, 3), (2, 3, 14, 64, 3), (5, 1, 16, 64, 3)], 1)
    # stride 2 with odd H / W, channel counts that are no multiple of 4, the stride-2 data-gradient test shapes
    rows += k3([(2, 9, 13, 64, 128), (1, 7, 5, 32, 32), (3, 13, 9, 6, 10), (1, 5, 7, 6, 10), (2, 24, 24, 64, 64), (1, 12, 12, 128, 64),
                (1, 6, 6, 256, 256), (1, 1, 8, 64, 64), (2, 10, 12, 66, 64)], 2)
    rows += k3([(1, 5, 7, 6, 10), (1, 5, 7, 8, 12), (3, 5, 7, 8, 8), (2, 7, 9, 30, 64)], 1)
    # both sides of the 2.5 GFLOP thresholds of the band / stride-1 tile weight-gradient kernels
    rows += k3([(1, 184, 184, 64, 64), (1, 188, 184, 64, 64), (2, 64, 64, 128, 128), (2, 68, 64, 128, 128), (1, 36, 36, 256, 256),
                (1, 40, 40, 256, 256)], 1)
    out, seen = [], set()
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(list(r))
    return out


def record(lib, shape_rows, names):
    def nm(b):
        s = b.decode()
        if s not in names:
            names.append(s)
        return names.index(s)
    table = []
    for B, H, W, cin, cout, k, s in shape_rows:
        shp = (B, H, W, cin, cout, k, s)
        row = [nm(lib.sst_conv_wgrad_kernel_name(*shp, 1))]
        row += [lib.sst_conv_wgrad_chunks2(*shp, n) for n in (1, 2, 16)]
        row += [lib.sst_conv_wgrad_pending_reduce(*shp, sc, act) for sc in (0, 1) for act in (0, 1)]
        row.append(lib.sst_conv_wgrad_groups_ok(*shp, max(1, B // 2)))
        row += [nm(lib.sst_conv_kernel_name(*shp, m, f)) for m in range(4) for f in range(2)]
        row.append(lib.sst_conv_stat_tiles(*shp))
        row += [nm(lib.sst_conv_s2_dgrad_kernel_name(B, H, W, cin, cout, f)) for f in (0, 1)]
        row.append(lib.sst_conv_s2_dgrad_tiles(B, H, W))
        table.append(row)
    return table


def tables(lib, shape_rows, names):
    """switch -> table; the switch is set alone, with sst_reload_env before and after."""
    out = {}
    for sw in SWITCHES:
        for k in [k for k in os.environ if k.startswith("SST_") and k != "SST_LIB_PATH"]:
            del os.environ[k]
        if sw:
            k, v = sw.split("=")
            os.environ[k] = v
        lib.sst_reload_env()
        out[sw] = record(lib, shape_rows, names)
    for sw in SWITCHES[1:]:
        os.environ.pop(sw.split("=")[0], None)
    lib.sst_reload_env()
    return out


def expand(doc):
    """The stored form keeps, per switch, only the rows that differ from the table without a switch."""
    full = {"": doc["base"]}
    for sw, diff in doc["switches"].items():
        full[sw] = [diff.get(str(i), row) for i, row in enumerate(doc["base"])]
    return full


def main():
    from srganst import _abi
    lib = _abi.lib()
    if "--mark-corrected" in sys.argv:
        doc = json.load(open(OUT))
        names = doc["names"]
        now, marks = tables(lib, doc["shapes"], names), {}
        for sw, want in expand(doc).items():
            for i, (w, g) in enumerate(zip(want, now[sw])):
                for c, (a, b) in enumerate(zip(w, g)):
                    if a != b:
                        if c not in NAME_COLS:
                            sys.exit(f"{sw or 'no switch'} {doc['shapes'][i]} {FIELDS[c]}: recorded {a}, library {b} - not a name: refusing")
                        marks.setdefault((i, FIELDS[c], names[a], names[b]), []).append(sw)
        marks = [{"row": i, "field": f, "name_corrected": True, "recorded": a, "name": b, "switches": sws} for (i, f, a, b), sws in marks.items()]
        doc["name_corrected"] = marks
    else:
        names = []
        shape_rows = shapes()
        t = tables(lib, shape_rows, names)
        doc = {"fields": FIELDS, "names": names, "shapes": shape_rows, "base": t[""],
               "switches": {sw: {str(i): r for i, r in enumerate(t[sw]) if r != t[""][i]} for sw in SWITCHES[1:]}, "name_corrected": []}
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": ' + _dump(v) for k, v in doc.items()) + "\n}\n")
    print(f"{OUT}: {len(doc['shapes'])} shapes, {os.path.getsize(OUT)} bytes, {len(doc['name_corrected'])} corrected names")


def _dump(v):
    if isinstance(v, dict):
        return "{\n" + ",\n".join(f'  "{k}": ' + json.dumps(x, separators=(",", ":")) for k, x in v.items()) + "\n }"
    if isinstance(v, list) and v and isinstance(v[0], (list, dict)):
        return "[\n" + ",\n".join("  " + json.dumps(x, separators=(",", ":")) for x in v) + "\n ]"
    return json.dumps(v)


if __name__ == "__main__":
    main()
