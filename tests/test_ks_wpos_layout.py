"""CPU check of k_mfma_ks's window-position layout (KS_WPOS; device_layout.cc wpos_step) through the
emitted program's binary sidecars.  A group is 8 position bytes + 8 values + one window byte: window
w is rows [5w, 5w + 5) of the wave image (halfwords [240w, 240w + 240) at the 48-halfword row
stride), a position byte the entry's halfword inside its group's window.  Checked: the codes and
window bytes are in range, the groups decode back to the plan's matrix exactly, padding inside a
live group repeats the group's first entry, all-padding groups write 0 into the zero row, the head
steps sit at their fixed slots, the layout is smaller than the u16 one by the margin that makes it
worth shipping, the C2 plan keeps MAXG = 1, and shapes the layout is not built for fall back."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import generalsparse_amd as gsa
from generalsparse_amd import datasets as ds

RS = 48        # halfwords per wave-image row (kKsStride / 2)
WIN_ROWS = 5   # image rows per window
WIN = WIN_ROWS * RS

M, K = 640, 2048
MATRICES = {
    "pruned": lambda: ds.pruned_weight(M, K, 0.7, 8),
    "random_rows": lambda: ds.random_rows(M, K, 400.0, seed=3, empty_frac=0.2),
}
_matrix_cache = {}


def _matrix(name):
    if name not in _matrix_cache:
        _matrix_cache[name] = MATRICES[name]()
    return _matrix_cache[name]


def _emit(tmp_path, m, k, r, c, v, rows, head, split=0, wpos=1, n=32):
    keys = ("HALF", "KS_HEAD", "KS_SPLIT", "KS_WPOS")
    old = {key: gsa.get_config(key) for key in keys}
    try:
        gsa.set_config("HALF", 1)
        gsa.set_config("KS_HEAD", head)
        gsa.set_config("KS_SPLIT", split)
        gsa.set_config("KS_WPOS", wpos)
        p = gsa.Plan.from_coo(m, k, r, c, v).run_pipeline("block_total", n, rows, 1).compile()
        d = p.generate_program(tmp_path, repeat=10)
        tbr = p.array("TBLOCK_META_first_row_indices_0").astype(np.int64)
    finally:
        for key, val in old.items():
            gsa.set_config(key, val)
    return d, tbr


def _launch(d):
    src = open(os.path.join(d, "kernel_file.hip")).read()
    m = re.search(r"gsk::k_mfma_ks<(\d+), (\d+), (\d+), (\d+), (\d+), false, (true|false), (false|true|gsk::kKsPosWin)", src)
    CT, RT, W, D, MAXG = map(int, m.groups()[:5])
    form = {"false": "kKsPosU16", "true": "kKsPos8"}.get(m.group(7), m.group(7)[5:])  # (the enum's 0 / 1)
    m = re.search(r"\(uint32_t\)K, N, (\d+)u, (\d+)u, (\d+)u, 0u, d_ws, d_arr, nullptr, (\d+)u(, d_win)?\)", src)
    S, NS, nwg, prio = map(int, m.groups()[:4])
    return dict(CT=CT, RT=RT, W=W, D=D, MAXG=MAXG, form=form, S=S, NS=NS, nwg=nwg, GH=(prio >> 8) & 0x3FF,
                win_arg=m.group(5) is not None)


def _sidecar_bytes(d, nb):
    """what the upload copies for the tiles: row-block rows (u32), positions, values, step records
    (and the window bytes)"""
    n = 4 * (nb + 1)
    for f in ("entry_pos", "entry_val", "steps", "group_win"):
        path = os.path.join(d, f"TBLOCK_META_mfma_ks_{f}_0.bin")
        if os.path.exists(path):
            n += os.path.getsize(path)
    return n


def _decode_wpos(d, m, k, tbr):
    L = _launch(d)
    assert L["form"] == "kKsPosWin" and L["win_arg"], L
    RT, W, D, S, NS, GH = L["RT"], L["W"], L["D"], L["S"], L["NS"], L["GH"]
    rd = lambda n, t: np.fromfile(os.path.join(d, n), dtype=t)
    steps = rd("TBLOCK_META_mfma_ks_steps_0.bin", np.uint32).reshape(-1, 2)
    pos = rd("TBLOCK_META_mfma_ks_entry_pos_0.bin", np.uint8).reshape(-1, 8).astype(np.int64)
    win = rd("TBLOCK_META_mfma_ks_group_win_0.bin", np.uint8).astype(np.int64)
    val = rd("TBLOCK_META_mfma_ks_entry_val_0.bin", np.uint16).reshape(-1, 8)
    assert len(pos) == len(win) == len(val)
    zrow = 16 * RT
    zwin = zrow // WIN_ROWS
    # every group: codes inside a window, windows up to the zero row's; image halfwords inside the image
    assert pos.max() < WIN and win.max() <= zwin
    half = win[:, None] * WIN + pos
    assert half.max() < (zrow + 1) * RS
    row, colw = half // RS, half % RS
    assert np.all(row // WIN_ROWS == win[:, None])  # a group lies in one window
    allpad = np.all(row == zrow, axis=1)
    # all-padding groups (head slots' spare groups, the spare group): value 0 into the zero row
    assert np.all(val[allpad] == 0) and np.all(win[allpad] == zwin)
    # live groups hold no zero-row entry, and any repeated place repeats the group's first entry
    live = ~allpad
    assert np.all(row[live] < zrow) and np.all(colw[live] < 32)
    assert allpad[-1], "the spare group"
    nb = len(tbr) - 1
    assert L["nwg"] == nb * S and len(steps) == nb * S * NS
    dense = np.zeros((m, k), np.float64)
    seen = np.zeros(len(pos), bool)
    HS = min(W * D, NS)
    valf = val.view(np.float16)
    gmax = 0
    for g in range(nb):
        R = tbr[g + 1] - tbr[g]
        for q in range(S):
            u = g * S + q
            for s in range(NS):
                first, cnt = (int(x) for x in steps[u * NS + s])
                gmax = max(gmax, cnt)
                if GH and s < HS:  # head steps at their fixed slots, all-padding groups after the entries
                    assert first == (u * HS + s) * GH and cnt <= GH, (u, s, first, cnt, GH)
                    assert np.all(allpad[first + cnt:first + GH])
                    seen[first:first + GH] = True
                assert not np.any(allpad[first:first + cnt])
                seen[first:first + cnt] = True
                for gi in range(first, first + cnt):
                    h = half[gi]
                    # padding repeats the first entry: position and value
                    _, idx = np.unique(h, return_index=True)
                    dup = np.ones(8, bool)
                    dup[idx] = False
                    assert np.all(h[dup] == h[0]) and np.all(val[gi][dup] == val[gi][0]), (gi, h, val[gi])
                    keep = np.sort(idx)
                    assert np.all(row[gi][keep] < R)
                    np.add.at(dense, (tbr[g] + row[gi][keep], q * NS * 32 + 32 * s + colw[gi][keep]),
                              valf[gi][keep].astype(np.float64))
    assert np.all(seen[:-1]) and not seen[-1]  # every group belongs to a step; the spare one to none
    return dense, L, gmax


def _reference(m, k, r, c, v):
    ref = np.zeros((m, k), np.float64)
    np.add.at(ref, (r.astype(np.int64), c.astype(np.int64)), v.astype(np.float16).astype(np.float64))
    return ref


@pytest.mark.parametrize("matrix", sorted(MATRICES))
@pytest.mark.parametrize("rows,split", [(40, 0), (40, 1), (112, 0), (80, 3), (56, 1)])
@pytest.mark.parametrize("head", [0, 1])
def test_wpos_layout_decodes_to_the_matrix(tmp_path, matrix, rows, split, head):
    r, c, v = _matrix(matrix)
    d, tbr = _emit(tmp_path, M, K, r, c, v, rows, head, split)
    dense, L, gmax = _decode_wpos(d, M, K, tbr)
    np.testing.assert_array_equal(dense, _reference(M, K, r, c, v))
    assert gmax <= 64 * L["MAXG"]
    if not head:
        assert L["GH"] == 0
    if matrix == "pruned":
        # the model says 0.83 of the u16 layout's bytes; 28 / 32 is the least worth shipping
        (tmp_path / "u16").mkdir()
        d16, tbr16 = _emit(tmp_path / "u16", M, K, r, c, v, rows, head, split, wpos=0)
        assert _launch(d16)["form"] == "kKsPosU16"
        b8, b16 = _sidecar_bytes(d, len(tbr) - 1), _sidecar_bytes(d16, len(tbr16) - 1)
        print(f"tile bytes: window positions {b8}, u16 {b16}, ratio {b8 / b16:.4f}")
        assert b8 < 0.875 * b16, (b8, b16)


def test_wpos_keeps_one_group_per_lane_on_the_c2_plan(tmp_path):
    """C2's plan: the windows' rounding up to whole groups must not spill a k-step past 64 groups
    (the model's largest step is 60)"""
    m = k = 5120
    r, c, v = ds.pruned_weight(m, k, 0.7, 13)
    d, tbr = _emit(tmp_path, m, k, r, c, v, 40, 1)
    L = _launch(d)
    assert L["form"] == "kKsPosWin" and (L["S"], L["NS"], L["W"], L["D"]) == (2, 80, 8, 2), L
    assert L["MAXG"] == 1 and 0 < L["GH"] <= 64, L
    steps = np.fromfile(os.path.join(d, "TBLOCK_META_mfma_ks_steps_0.bin"), dtype=np.uint32).reshape(-1, 2)
    assert steps[:, 1].max() <= 64
    nnz = len(r)
    b8 = _sidecar_bytes(d, len(tbr) - 1)
    print(f"C2: {b8} tile bytes, {b8 / nnz:.3f} B per nonzero, largest step {steps[:, 1].max()} groups, GH {L['GH']}")


def test_wpos_falls_back_on_an_unsupported_width(tmp_path):
    """N = 128 is not a window-position shape: the u16 layout, no window sidecar"""
    r, c, v = _matrix("pruned")
    d, _ = _emit(tmp_path, M, K, r, c, v, 40, 1, n=128)
    L = _launch(d)
    assert L["form"] == "kKsPosU16" and not L["win_arg"], L
    assert not os.path.exists(os.path.join(d, "TBLOCK_META_mfma_ks_group_win_0.bin"))


def test_release_build_refuses_pos8_and_accepts_wpos_from_json(tmp_path):
    """KS_POS8 stays an experiments-build switch, refused from a JSON config; KS_WPOS is a release key"""
    from build_flags import EXPERIMENTS
    if EXPERIMENTS:
        pytest.skip("the experiments build accepts KS_POS8")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import generalsparse_amd as g\n"
            "try:\n    print('KS_WPOS', g.get_config('KS_WPOS'))\nexcept g.GsError as e:\n    print('REFUSED', e)\n")
    cfg = tmp_path / "cfg.json"
    cfg.write_text('{"HALF": true, "KS_POS8": 1}\n')
    env = dict(os.environ, GS_CONFIG=str(cfg))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=root)
    assert "REFUSED" in out.stdout and "KS_POS8" in out.stdout, out.stdout + out.stderr
    cfg.write_text('{"HALF": true, "KS_WPOS": 1}\n')
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=root)
    assert "KS_WPOS 1" in out.stdout, out.stdout + out.stderr
