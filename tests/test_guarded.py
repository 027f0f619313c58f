"""tests/guarded.py on CPU tensors: the evidence that the guard-band and bit-exact checks of the
GPU edge tests bite (no kernel is altered on the GPU to show it)."""
import pytest

torch = pytest.importorskip("torch")
import guarded as gd  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
SHAPES = [(203, 1), (203, 5), (131, 67), (33, 520)]


def small_ints(rows, cols, dtype, seed=0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randint(-2, 3, (rows, cols), generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_payload_views(rows, cols, dtype):
    src = small_ints(rows, cols, dtype)
    B, hb = gd.guarded_B(src, "cpu")
    C, hc = gd.guarded_C(rows, cols, dtype, "cpu")
    for t, h in ((B, hb), (C, hc)):
        assert tuple(t.shape) == (rows, cols) and t.is_contiguous() and t.dtype == dtype
        assert h.G % 128 == 0 and h.G >= 128 * cols
        assert h.flat.numel() == 2 * h.G + rows * cols
        assert (t.data_ptr() - h.flat.data_ptr()) % 256 == 0
        assert t.data_ptr() - h.flat.data_ptr() == h.G * t.element_size()
        assert t.data_ptr() == h.payload.data_ptr()
    assert torch.equal(B, src)
    n = rows * cols
    assert hb.flat[:hb.G].isnan().all() and hb.flat[hb.G + n:].isnan().all()
    assert C.isnan().all()
    bands = torch.cat([hc.flat[:hc.G], hc.flat[hc.G + n:]])
    assert torch.isfinite(bands).all() and (bands != 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_untouched_operands_pass(dtype):
    src = small_ints(40, 13, dtype)
    B, hb = gd.guarded_B(src, "cpu")
    C, hc = gd.guarded_C(40, 13, dtype, "cpu")
    C.copy_(src)  # a kernel that writes all of C and nothing else
    gd.assert_guards_intact(hb, "B")
    gd.assert_guards_intact(hc, "C")
    gd.assert_bits(C, src, "C")
    hc.refill()
    assert C.isnan().all()
    gd.assert_guards_intact(hc, "C refilled")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("where,row,col", [("after", 40, 0), ("after", 40, 5), ("after", 41, 12), ("before", -1, 12),
                                           ("before", -3, 4), ("last", None, None), ("first", None, None)])
def test_altered_band_word_is_named(where, row, col, dtype):
    M, N = 40, 13
    C, h = gd.guarded_C(M, N, dtype, "cpu")
    if where == "last":
        idx = h.flat.numel() - 1
        off = idx - h.G
        row, col = off // N, off % N
    elif where == "first":
        idx = 0
        row, col = (-h.G) // N, (-h.G) % N
    else:
        idx = h.G + row * N + col
    h.flat[idx] = 0.0  # one stray store
    with pytest.raises(AssertionError) as ex:
        gd.assert_guards_intact(h, "stray")
    msg = str(ex.value)
    assert f"row {row}, column {col} " in msg and f"offset {row * N + col} " in msg, msg
    assert ("low" if row < 0 else "high") in msg and "stray" in msg, msg


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_altered_band_bit_is_seen(dtype):
    """one flipped low mantissa bit (the bands are compared as integers, not as floats), and a
    NaN band of B whose payload bits change while it stays NaN"""
    C, h = gd.guarded_C(7, 24, dtype, "cpu")
    iv = h.flat.view(gd._int_dtype(h.flat))
    iv[h.G + 7 * 24 + 3] ^= 1
    with pytest.raises(AssertionError, match="row 7, column 3 "):
        gd.assert_guards_intact(h)
    B, hb = gd.guarded_B(small_ints(7, 24, dtype), "cpu")
    ib = hb.flat.view(gd._int_dtype(hb.flat))
    ib[hb.G - 1] ^= 1
    assert hb.flat[hb.G - 1].isnan()
    with pytest.raises(AssertionError, match="row -1, column 23 "):
        gd.assert_guards_intact(hb)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_altered_payload_element_fails_bit_exact(dtype):
    ref = small_ints(40, 13, dtype)
    C, h = gd.guarded_C(40, 13, dtype, "cpu")
    C.copy_(ref)
    gd.assert_bits(C, ref, "same")
    C[17, 5] = ref[17, 5] + 1
    with pytest.raises(AssertionError, match=r"1 elements differ"):
        gd.assert_bits(C, ref, "one off")
    C.copy_(ref)
    C[39, 12] = float("nan")  # an element no kernel wrote
    with pytest.raises(AssertionError, match=r"1 elements differ"):
        gd.assert_bits(C, ref, "unwritten")
    C.copy_(ref)
    z = (ref == 0).nonzero()[0].tolist()
    C[z[0], z[1]] = -0.0  # equal as a float, another bit pattern
    with pytest.raises(AssertionError, match=r"1 elements differ"):
        gd.assert_bits(C, ref, "minus zero")


def test_sixteen_bit_types_use_the_shared_checker():
    """assert_bits on fp16 / bf16 is tests/test_gpu_exact.py's assert_bit_exact, not a copy"""
    import test_gpu_exact as ex
    assert gd.assert_bit_exact is ex.assert_bit_exact and gd.int_values is ex.int_values
