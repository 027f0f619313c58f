"""bfloat16 as a plan dtype, host side (no GPU): the GS_BF16 code, its spellings, and
gs_convert_values -- the conversion gs_plan_upload applies to A's values -- against torch's
float32 -> bfloat16 (round to nearest even) bit for bit, and against numpy for fp16."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402


def bits_to_f32(b):
    return np.asarray(b, np.uint32).view(np.float32)


def torch_bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def finite_inputs():
    """the named input classes, each a float32 array of finite values"""
    rng = np.random.default_rng(2024)
    normals = (rng.standard_normal(100_000) * np.exp2(rng.integers(-60, 61, 100_000))).astype(np.float32)
    # every tie: upper half k (even and odd, both signs, denormals included), lower half exactly 1/2 ulp
    k = np.arange(0, 0x7f80, dtype=np.uint32)
    ties = bits_to_f32(np.concatenate([(k << 16) | 0x8000, (k << 16) | 0x8000 | 0x80000000]))
    just_under = bits_to_f32(np.concatenate([(k << 16) | 0x7fff, (k << 16) | 0x8001]))
    zeros = bits_to_f32([0x00000000, 0x80000000])
    denormals = bits_to_f32([0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff, 0x80000001,
                             0x80008000, 0x807fffff, 0x00400000])
    # around bf16's largest finite value 0x7f7f: the next fp32 above it still rounds to it, the
    # halfway point and everything above round to Inf
    top = bits_to_f32([0x7f7f0000, 0x7f7f0001, 0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7f8000, 0xff7fffff])
    return {"normals": normals, "ties": ties, "near_ties": just_under, "zeros": zeros, "denormals": denormals, "top": top}


def test_bf16_code_and_spellings():
    assert gsa.GS_BF16 == 2 and "GS_BF16" in gsa.__all__
    for spelling in (gsa.GS_BF16, "bf16", "bfloat16", torch.bfloat16):
        assert gsa._dtype_code(spelling) == 2, spelling
    assert gsa._dtype_code("f16") == gsa.GS_F16 == 1 and gsa._dtype_code("f32") == gsa.GS_F32 == 0
    for bad in ("bf8", "int8", 3, torch.float64, None):
        with pytest.raises(ValueError):
            gsa._dtype_code(bad)


def test_three_way_operand_table():
    assert [gsa._torch_dtype(c) for c in (gsa.GS_F32, gsa.GS_F16, gsa.GS_BF16)] == \
        [torch.float32, torch.float16, torch.bfloat16]


@pytest.mark.parametrize("name", ["normals", "ties", "near_ties", "zeros", "denormals", "top"])
def test_convert_values_bf16_is_torch_rne(name):
    x = finite_inputs()[name]
    got = gsa.convert_values(x, "bf16")
    assert got.dtype == np.uint16 and got.shape == x.shape
    np.testing.assert_array_equal(got, torch_bf16_bits(x))


def test_convert_values_bf16_specials():
    inf = np.array([np.inf, -np.inf], np.float32)
    np.testing.assert_array_equal(gsa.convert_values(inf, "bf16"), np.array([0x7f80, 0xff80], np.uint16))
    # the first fp32 values past bf16's largest finite one that RNE sends to Inf
    over = bits_to_f32([0x7f7f8000, 0x7f7fffff, 0xff7f8000])
    np.testing.assert_array_equal(gsa.convert_values(over, "bf16"), np.array([0x7f80, 0x7f80, 0xff80], np.uint16))
    # ... and the one just above the largest finite value stays there
    np.testing.assert_array_equal(gsa.convert_values(bits_to_f32([0x7f7f0001]), "bf16"), np.array([0x7f7f], np.uint16))
    nans = bits_to_f32([0x7fc00000, 0xffc00000, 0x7f800001, 0x7f80ffff, 0xff800001, 0x7fffffff])
    got = gsa.convert_values(nans, "bf16")
    back = torch.from_numpy(got.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.isnan(back).all(), got
    assert ((got & 0x0040) != 0).all(), got  # quiet
    # the ladder the GPU rounding test uses: 257 -> 256, 259 -> 260, 261 -> 260, 263 -> 264
    ladder = np.array([255, 256, 257, 258, 259, 261, 263, 511, 513, 1025], np.float32)
    back = torch.from_numpy(gsa.convert_values(ladder, "bf16").view(np.int16)).view(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(back, [255, 256, 256, 258, 260, 260, 264, 512, 512, 1024])


@pytest.mark.parametrize("name", ["normals", "ties", "near_ties", "zeros", "denormals", "top"])
def test_convert_values_f16_is_numpy(name):
    x = finite_inputs()[name]
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    np.testing.assert_array_equal(gsa.convert_values(x, "f16"), want)


def test_convert_values_f32_is_identity_and_bad_dtype_is_refused():
    x = np.concatenate(list(finite_inputs().values()))
    got = gsa.convert_values(x, "f32")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), x.view(np.uint32))
    assert gsa.convert_values(np.zeros(0, np.float32), "bf16").size == 0
    L = gsa.load_library()
    out = np.zeros(4, np.uint16)
    import ctypes
    for bad in (3, -1, 7):
        rc = L.gs_convert_values(np.ones(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 4, bad,
                                 ctypes.c_void_p(out.ctypes.data))
        assert rc == -1 and b"dtype" in L.gs_last_error()
    assert not out.any()


def test_upload_refuses_an_unknown_dtype_before_touching_a_device():
    """gs_plan_upload takes 0, 1 and 2 only (the check precedes every device call)"""
    from generalsparse_amd import datasets as ds
    row, col, val = ds.random_rows(64, 64, 6.0, seed=1)
    plan = gsa.Plan.from_coo(64, 64, row, col, val).run_pipeline("thread_total", 8, 4, 1).compile()
    rc = plan._L.gs_plan_upload(plan._h, 3, 0)
    assert rc == -1 and b"bf16" in plan._L.gs_last_error()
