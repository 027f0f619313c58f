"""CPU checks of the FP8 (OCP e4m3fn) weight values of k_mfma_ks plans (Plan.upload(weights="fp8")):
the decode table, the quantiser (default power-of-two scales and supplied ones, ties to even,
saturation, refusals) against torch.float8_e4m3fn, and the 8-bit value array of the upload layout
(Plan.fp8_layout, no device) against the emitted f16 program's groups."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from generalsparse_amd import datasets as ds  # noqa: E402
from test_ks_layout import RS, _emit  # noqa: E402

FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)


def torch_decode(codes):
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn).float().numpy()


def torch_codes(x):
    """(x: float32 numpy).to(float8_e4m3fn) as bytes"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ------------------------------------------------------------------ decode
def test_decode_is_torchs_on_every_finite_code():
    assert len(FINITE) == 254
    got = gsa.fp8_decode(np.arange(256, dtype=np.uint8))
    assert got.dtype == np.float32 and got.shape == (256,)
    np.testing.assert_array_equal(got[FINITE].view(np.uint32), torch_decode(FINITE).view(np.uint32))  # -0 too
    assert np.isnan(got[0x7F]) and np.isnan(got[0xFF])
    # every finite e4m3 value is an fp16 value: what lets the kernel decode to fp16 and run the f16 MFMAs
    np.testing.assert_array_equal(got[FINITE].astype(np.float16).astype(np.float32), got[FINITE])
    assert np.abs(got[FINITE]).max() == 448.0


# ------------------------------------------------------------------ quantise, default scales
def test_default_scale_rule_on_hand_rows():
    val = np.array([2.0, -1.0, 448.0, 3.0, 449.0, 0.0, 0.0, 224.0, 225.0, -7.0], np.float32)
    row = np.array([0, 0, 1, 1, 2, 3, 3, 5, 6, 7])
    codes, scale = gsa.fp8_quantize(val, row, 9)
    #          amax 2 -> 2^-7, 448 -> 1, 449 -> 2, a zero row -> 1, no value -> 1, 224 -> 2^-1, 225 -> 1, 7 -> 2^-6, none
    want = [2.0 ** -7, 1.0, 2.0, 1.0, 1.0, 0.5, 1.0, 2.0 ** -6, 1.0]
    np.testing.assert_array_equal(scale, np.array(want, np.float32))
    assert codes.dtype == np.uint8 and scale.dtype == np.float32
    q = np.abs(val) / scale[row]
    amax = np.array([q[row == r].max() if (row == r).any() else 0.0 for r in range(9)])
    live = amax > 0
    assert ((amax[live] > 224) & (amax[live] <= 448)).all(), amax
    np.testing.assert_array_equal(codes, torch_codes(val / scale[row]))


def test_default_scales_match_torch_byte_for_byte():
    rng = np.random.default_rng(11)
    n_rows, per = 97, 300
    row = np.repeat(np.arange(n_rows), per)
    val = (rng.standard_normal(n_rows * per) * np.exp2(rng.integers(-20, 20, n_rows))[row]).astype(np.float32)
    val[rng.random(val.size) < 0.02] = 0.0
    val[5 * per:6 * per] = 0.0  # a row of zeros
    codes, scale = gsa.fp8_quantize(val, row, n_rows + 1)  # the last row holds no value
    assert scale[5] == 1.0 and scale[n_rows] == 1.0
    m, e = np.frexp(scale)
    assert (m == 0.5).all(), "power-of-two scales"
    amax = np.abs(val).reshape(n_rows, per).max(1)
    live = amax > 0
    ratio = amax[live] / scale[:n_rows][live]
    assert ((ratio > 224) & (ratio <= 448)).all()
    np.testing.assert_array_equal(codes, torch_codes(val / scale[row]))
    assert not np.isin(codes, [0x7F, 0xFF]).any()
    # the dequantised value is within half a code step of the value
    back = gsa.fp8_decode(codes) * scale[row]
    assert (np.abs(back - val) <= np.abs(val) * 2.0 ** -4 + scale[row] * 2.0 ** -10).all()


def test_ties_round_to_even():
    """the exact midpoints between neighbouring codes (scale 1): ties go to the even code"""
    pos = np.array([c for c in range(0x7F)], np.uint8)  # 0 .. 0x7e: ascending values
    v = gsa.fp8_decode(pos).astype(np.float64)
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)
    assert (mid.astype(np.float64) == (v[:-1] + v[1:]) / 2).all()  # exact in fp32
    for sign in (1.0, -1.0):
        codes, scale = gsa.fp8_quantize(sign * mid, np.zeros(len(mid), np.int64), 1, row_scale=[1.0])
        want = np.where(pos[:-1] % 2 == 0, pos[:-1], pos[1:]) | (0x80 if sign < 0 else 0)
        np.testing.assert_array_equal(codes, want.astype(np.uint8))
        np.testing.assert_array_equal(codes, torch_codes(sign * mid))
        # and just beside the midpoint the nearer code wins
        up = np.nextafter(mid, np.float32(np.inf))
        dn = np.nextafter(mid, np.float32(-np.inf))
        np.testing.assert_array_equal(gsa.fp8_quantize(sign * up, np.zeros(len(mid), np.int64), 1, row_scale=[1.0])[0] & 0x7F, pos[1:])
        np.testing.assert_array_equal(gsa.fp8_quantize(sign * dn, np.zeros(len(mid), np.int64), 1, row_scale=[1.0])[0] & 0x7F, pos[:-1])


# ------------------------------------------------------------------ quantise, supplied scales
def test_supplied_scales_match_torch_within_range():
    rng = np.random.default_rng(12)
    n_rows, per = 53, 200
    row = np.repeat(np.arange(n_rows), per)
    val = (rng.standard_normal(n_rows * per) * rng.uniform(0.01, 30.0, n_rows)[row]).astype(np.float32)
    amax = np.abs(val).reshape(n_rows, per).max(1)
    scale_in = (amax / np.float32(448.0)).astype(np.float32)  # not powers of two
    q = val / scale_in[row]
    keep = np.abs(q) <= 448  # (the fp32 quotient of the row's amax may land a bit above: saturation, below)
    assert keep.mean() > 0.99
    codes, scale = gsa.fp8_quantize(val, row, n_rows, row_scale=scale_in)
    np.testing.assert_array_equal(scale, scale_in)
    np.testing.assert_array_equal(codes[keep], torch_codes(q[keep]))
    assert (np.abs(gsa.fp8_decode(codes)) <= 448).all()


def test_saturation_at_448():
    val = np.array([448.0, 449.0, 464.0, 465.0, 480.0, 1e6, 3e38, -449.0, -465.0, -1e30, 447.0, 1e-10, -1e-10], np.float32)
    codes, _ = gsa.fp8_quantize(val, np.zeros(len(val), np.int64), 1, row_scale=[1.0])
    want = np.array([448.0] * 7 + [-448.0] * 3 + [448.0, 0.0, -0.0], np.float32)
    np.testing.assert_array_equal(gsa.fp8_decode(codes), want)
    assert codes[-1] == 0x80 and codes[-2] == 0x00
    codes, _ = gsa.fp8_quantize([1.0, -1.0], [0, 0], 1, row_scale=[1e-38])  # the quotient overflows fp32
    np.testing.assert_array_equal(codes, np.array([0x7E, 0xFE], np.uint8))


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_values_are_refused(bad):
    with pytest.raises(gsa.GsError, match="non-finite"):
        gsa.fp8_quantize([1.0, bad, 2.0], [0, 1, 1], 2)
    with pytest.raises(gsa.GsError, match="non-finite"):
        gsa.fp8_quantize([1.0, bad, 2.0], [0, 1, 1], 2, row_scale=[1.0, 1.0])


@pytest.mark.parametrize("scales", [[1.0, 0.0], [1.0, -2.0], [np.nan, 1.0], [np.inf, 1.0], [1.0], [1.0, 1.0, 1.0]])
def test_bad_scales_are_refused(scales):
    with pytest.raises(gsa.GsError, match="scale"):
        gsa.fp8_quantize([1.0, 2.0], [0, 1], 2, row_scale=scales)


def test_bad_rows_are_refused():
    with pytest.raises(gsa.GsError):
        gsa.fp8_quantize([1.0, 2.0], [0, 2], 2)
    with pytest.raises(gsa.GsError):
        gsa.fp8_quantize([1.0, 2.0], [0], 2)
    with pytest.raises(ValueError):
        gsa.Plan.from_coo(2, 2, [0, 1], [0, 1], [1.0, 1.0]).upload("f16", 0, weights="int4")


# ------------------------------------------------------------------ layout
def representable_weight(M, K, seed):
    """a 70%-pruned M x K weight whose values are e4m3 codes times a per-row power of two: every row
    holds a value of magnitude in (224, 448] codes, so the default scale of row r is exactly pw[r]"""
    r, c, _ = ds.pruned_weight(M, K, 0.7, seed)
    rng = np.random.default_rng(seed)
    live = FINITE[(FINITE & 0x7F) != 0]  # no zero codes: every stored entry keeps a non-zero value
    code = rng.choice(live, len(r))
    first = np.unique(r, return_index=True)[1]
    code[first] = rng.choice(np.arange(0x77, 0x7F, dtype=np.uint8), len(first))  # 240 .. 448
    pw = np.exp2(rng.integers(-6, 4, M)).astype(np.float32)
    v = gsa.fp8_decode(code) * pw[r.astype(np.int64)]
    assert (v.astype(np.float16).astype(np.float32) == v).all() and (v != 0).all()
    return r, c, v.astype(np.float32), pw


@pytest.mark.parametrize("rows,split", [(40, 0), (40, 3), (80, 0), (80, 3)])
@pytest.mark.parametrize("head", [0, 1])
def test_fp8_layout_is_the_f16_layout_slot_for_slot(tmp_path, rows, split, head):
    """the emitted f16 program's groups (positions, f16 values) against the accessor's 8-bit array of the
    same plan under the same config: decode(code) * scale[row of the slot] is the slot's f16 value at
    every live slot, and every pad slot (a position in the image's zero row) holds code 0"""
    M, K = 640, 4096
    r, c, v, pw = representable_weight(M, K, 51)
    d, tbr = _emit(tmp_path, M, K, r, c, v, rows, head, split)
    keys = ("HALF", "KS_HEAD", "KS_SPLIT")
    old = {k: gsa.get_config(k) for k in keys}
    try:
        for k, x in zip(keys, (1, head, split)):
            gsa.set_config(k, x)
        plan = gsa.Plan.from_coo(M, K, r, c, v).run_pipeline("block_total", 32, rows, 1).compile()
        codes, scale = plan.fp8_layout()
    finally:
        for k, x in old.items():
            gsa.set_config(k, x)
    np.testing.assert_array_equal(scale, pw)
    import os
    import re
    src = open(os.path.join(d, "kernel_file.hip")).read()
    RT = int(re.search(r"gsk::k_mfma_ks<(\d+), (\d+),", src).group(2))
    S, NS = map(int, re.search(r"\(uint32_t\)K, N, (\d+)u, (\d+)u,", src).groups())
    pos = np.fromfile(os.path.join(d, "TBLOCK_META_mfma_ks_entry_pos_0.bin"), np.uint16).astype(np.int64)
    val = np.fromfile(os.path.join(d, "TBLOCK_META_mfma_ks_entry_val_0.bin"), np.uint16).view(np.float16).astype(np.float32)
    steps = np.fromfile(os.path.join(d, "TBLOCK_META_mfma_ks_steps_0.bin"), np.uint32).reshape(-1, 2).astype(np.int64)
    assert codes.shape == pos.shape == val.shape and len(codes) % 8 == 0
    pad = pos // RS == 16 * RT  # the zero row
    assert (codes[pad] == 0).all() and (val[pad] == 0).all() and pad.any()
    # the row block of every group, from the step records (head slots' spare groups and the spare group: all pads)
    nb = len(tbr) - 1
    assert len(steps) == nb * S * NS
    block = np.full(len(codes) // 8, -1, np.int64)
    for u in range(nb * S):
        for first, cnt in steps[u * NS:(u + 1) * NS]:
            block[first:first + cnt] = u // S
    slot_block = np.repeat(block, 8)
    assert (slot_block[~pad] >= 0).all()
    row_of = tbr[slot_block[~pad]] + pos[~pad] // RS
    assert (row_of < M).all() and (~pad).sum() == len(r)
    np.testing.assert_array_equal(gsa.fp8_decode(codes[~pad]) * scale[row_of], val[~pad])


def test_fp8_layout_refusals():
    M, K = 640, 4096
    r, c, v, _ = representable_weight(M, K, 52)
    plan = gsa.Plan.from_coo(M, K, r, c, v).run_pipeline("block_total", 64, 40, 1).compile()
    with pytest.raises(gsa.GsError, match="17 .. 32"):
        plan.fp8_layout()
    plan = gsa.Plan.from_coo(M, K, r, c, v).run_pipeline("thread_total", 32, 4, 1).compile()
    with pytest.raises(gsa.GsError, match="k_mfma_ks"):
        plan.fp8_layout()
    v2 = v.copy()
    v2[7] = np.nan
    plan = gsa.Plan.from_coo(M, K, r, c, v2).run_pipeline("block_total", 32, 40, 1).compile()
    with pytest.raises(gsa.GsError, match="non-finite"):
        plan.fp8_layout()
    plan = gsa.Plan.from_coo(M, K, r, c, v).run_pipeline("block_total", 32, 40, 1).compile()
    with pytest.raises(gsa.GsError, match="scale"):
        plan.fp8_layout(row_scale=np.zeros(M, np.float32))
    with pytest.raises(gsa.GsError):
        plan.fp8_layout(row_scale=np.ones(M - 1, np.float32))
    codes, scale = plan.fp8_layout(row_scale=np.full(M, 0.75, np.float32))
    assert (scale == 0.75).all() and len(codes) % 8 == 0
