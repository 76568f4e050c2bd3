"""CPU self-check of tests/guards.py: the checker has teeth (a single element written into a band or a pad is reported with the
right location), an untouched poisoned buffer passes, and the views have the leading dimension and alignment that was asked."""

import pytest
import torch

from tests import guards

CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype,fill", [(torch.float32, None), (torch.bfloat16, None), (torch.uint8, "fp8"), (torch.uint8, "e8m0"),
                                        (torch.int32, None), (torch.int64, None), (torch.uint8, None), (torch.int16, None)])
def test_untouched_buffer_passes_and_holds_the_poison(dtype, fill):
    view, chk = guards.guarded((5, 24), dtype, CPU, ld=32, fill=fill)
    chk()                                                   # NaN bands compare equal to themselves: bits, not floats
    flat = chk.flat
    band, pad = flat[: chk.front], flat[chk.front: chk.front + 5 * 32].view(5, 32)[:, 24:]
    if dtype.is_floating_point:
        assert torch.isnan(band.float()).all() and torch.isnan(pad.float()).all() and torch.isnan(view.float()).all()
        assert torch.isnan(flat[chk.front + 5 * 32:].float()).all()
    else:
        want = {"fp8": 0x7F, "e8m0": 0xFF, None: guards.INT_PATTERN}[fill]
        assert (band.view(torch.uint8) == want).all() and (pad.contiguous().view(torch.uint8) == want).all()
    view.fill_(1)                                           # writing the view of an OUTPUT is what a kernel is for
    chk()


@pytest.mark.parametrize("ld", [24, 32, 64])
@pytest.mark.parametrize("dtype,align", [(torch.float32, 16), (torch.bfloat16, 16), (torch.uint8, 4), (torch.uint8, 16), (torch.float32, 4)])
def test_view_geometry(dtype, align, ld):
    view, chk = guards.guarded((7, 24), dtype, CPU, ld=ld, align=align)
    esz = view.element_size()
    assert tuple(view.shape) == (7, 24) and view.stride() == (ld, 1)
    off = view.data_ptr() - chk.flat.data_ptr()
    assert off % align == 0 and off % (2 * align) == align          # exactly the documented alignment, nothing stricter
    band = chk.front - align // esz
    assert band * esz >= guards.BAND_BYTES and band >= guards.BAND_ROWS * ld
    assert chk.flat.numel() - chk.front - 7 * ld == band            # the same band behind
    v3, c3 = guards.guarded((2, 3, 8), torch.float32, CPU, ld=12)   # leading dimensions fold into rows
    assert v3.stride() == (36, 12, 1) and c3.rows == 6
    v1, c1 = guards.guarded(10, torch.float32, CPU)                 # a flat buffer is one row
    assert tuple(v1.shape) == (10,) and (c1.rows, c1.cols, c1.ld) == (1, 10, 10)


def test_wide_rows_get_256_rows_of_band():
    _, chk = guards.guarded((3, 1000), torch.float32, CPU, ld=1040)
    assert chk.front >= 256 * 1040 and chk.flat.numel() - chk.front - 3 * 1040 >= 256 * 1040


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int32])
def test_single_element_writes_are_located(dtype):
    M, N, ld = 6, 20, 28  # noqa: N806
    cases = [(-1, "front band: row -1, pad col N+7"),                # the element just in front of the view
             (-ld, "front band: row -1, col 0"),
             (-ld - 5, "front band: row -2, pad col N+3"),
             (M * ld, "back band: row M+0, col 0"),
             (M * ld + 17, "back band: row M+0, col 17"),
             ((M + 2) * ld + N + 1, "back band: row M+2, pad col N+1"),
             (3 * ld + N, "pad col N+0 of row 3"),
             (5 * ld + N + 3, "pad col N+3 of row 5"),                # the last row's pad, in front of the back band
             (0 * ld + ld - 1, "pad col N+7 of row 0")]
    for off, want in cases:
        view, chk = guards.guarded((M, N), dtype, CPU, ld=ld, fill="fp8" if dtype == torch.uint8 else None)
        chk.flat[chk.front + off] = 1
        hit = chk.first_change()
        assert hit is not None and hit[0] == want, (off, hit, want)
        with pytest.raises(AssertionError, match="changed at"):
            chk()
    view, chk = guards.guarded((M, N), dtype, CPU, ld=ld)            # the far ends of both bands
    chk.flat[0] = 1
    assert chk.first_change()[0].startswith("front band")
    view, chk = guards.guarded((M, N), dtype, CPU, ld=ld)
    chk.flat[-1] = 1
    assert chk.first_change()[0].startswith("back band")


def test_nan_to_other_nan_is_a_change_and_zero_sign_too():
    view, chk = guards.guarded((4, 8), torch.float32, CPU, ld=16)
    bits = chk.flat.view(torch.int32)
    bits[chk.front + 4 * 16] ^= 1                                    # still a NaN, other payload: a float compare cannot see it
    assert torch.isnan(chk.flat[chk.front + 4 * 16])
    assert chk.first_change()[0] == "back band: row M+0, col 0"
    data = torch.zeros(2, 4)
    view, chk = guards.guarded((2, 4), torch.float32, CPU, data=data)
    view[1, 3] = -0.0                                                # equal as a float, other bits
    assert chk.first_change()[0] == "row 1, col 3"


def test_inputs_must_keep_their_own_bits():
    data = torch.arange(12, dtype=torch.float32).view(3, 4)
    view, chk = guards.guarded((3, 4), torch.float32, CPU, ld=8, data=data)
    assert torch.equal(view, data)
    chk()
    view[1, 2] = -0.0 if float(view[1, 2]) == 0 else 77.0
    assert chk.first_change()[0] == "row 1, col 2"
    out, ochk = guards.guarded((3, 4), torch.float32, CPU, ld=8, init=0.0)
    assert (out == 0).all()
    out[1, 2] = 5.0
    ochk()                                                           # an output's interior is free


def test_trap_index_bands_hold_a_valid_index():
    idx = torch.tensor([[3, 1, 4], [1, 5, 2]], dtype=torch.int32)
    view, chk = guards.trap_index(idx, 9, CPU, ld=4)
    assert torch.equal(view, idx)
    flat = chk.flat
    interior = chk._interior()
    assert (flat[~interior] == 9).all()                              # every element around the view is the trap index
    src = torch.cat([torch.ones(9, 2), torch.full((1, 2), float("nan"))])
    over = flat[chk.front + 3]                                       # what a kernel reading one index too many of row 0 gets
    assert torch.isnan(src[int(over)]).all()
    chk.flat[chk.front - 1] = 0
    assert chk.first_change()[0] == "front band: row -1, pad col N+0"
    spans = torch.tensor([[0, 5], [7, 3]], dtype=torch.int64)        # records: the trap is a whole valid record, tiled in phase
    sv, schk = guards.trap_index(spans, [100, 1], CPU)
    assert torch.equal(sv, spans)
    assert schk.flat[schk.front - 2: schk.front].tolist() == [100, 1]
    assert schk.flat[schk.front + 4: schk.front + 8].tolist() == [100, 1, 100, 1]


def test_guard_set_checks_every_buffer():
    gs = guards.GuardSet(CPU)
    a = gs.inp(torch.ones(3, 8), ld=16, name="a")
    b = gs.out((3, 8), torch.bfloat16, ld=16, name="b")
    gs.check()
    b.fill_(2.0)
    gs.check()
    assert a.stride() == (16, 1) and b.stride() == (16, 1)
    gs.guards[1].flat[gs.guards[1].front + 8] = 0                    # pad column of b's first row
    with pytest.raises(AssertionError, match=r"b: guard band changed at pad col N\+0 of row 0"):
        gs.check()
