"""CPU tests of the argument layer of the record calls' binding (rejit_amd/api.py: the private helpers above class Scan).  The
helpers take tensors of any torch device, so CPU tensors and a stub `call` that records its arguments and returns a scripted
total pin the host protocol every record method shares: the row list whose empty form must not read as "every row", the
size-query-then-fill of a new device text, the one-byte argument and the pointer of a tensor."""
import ctypes

import pytest
import torch

from rejit_amd import api

CPU = torch.device("cpu")


def address(p):
    assert isinstance(p, ctypes.c_void_p)
    return p.value or 0


def test_pointer_of_none_and_of_an_empty_tensor_is_null():
    assert address(api._ptr(None)) == 0
    assert address(api._ptr(torch.empty(0, dtype=torch.uint8))) == 0
    t = torch.zeros(3, dtype=torch.int64)
    assert address(api._ptr(t)) == t.data_ptr() != 0


def test_row_list_none_is_every_row():
    assert api._rows(None, 7, CPU) == (None, 7)


def test_row_list_empty_is_a_non_null_pointer_and_no_rows():
    empty = torch.empty(0, dtype=torch.int64)
    passed, k = api._rows(empty, 7, CPU)
    assert k == 0
    assert passed.dtype == torch.int64 and passed.numel() == 1 and passed.device == CPU
    where = address(api._ptr(passed))
    assert where != 0
    del empty
    assert passed.data_ptr() == where and int(passed[0]) == 0      # the tensor is the caller's to hold, and it holds


def test_row_list_is_passed_through():
    idx = torch.tensor([3, 0, 0, 2])
    passed, k = api._rows(idx, 7, CPU)
    assert passed is idx and k == 4


def test_row_list_refuses_a_strided_list_and_another_dtype():
    with pytest.raises(AssertionError):
        api._rows(torch.arange(8)[::2], 7, CPU)
    with pytest.raises(AssertionError):
        api._rows(torch.tensor([3, 0], dtype=torch.int32), 7, CPU)


class Stub:
    """call(buf, cap) -> the scripted total; keeps (buf, cap) of every call"""

    def __init__(self, total):
        self.total, self.calls = total, []

    def __call__(self, buf, cap):
        self.calls.append((buf, cap))
        return self.total


def sized(call, out):
    return api._sized_text(call, out, CPU, "pack_records", "the packed text")


def test_sized_text_of_no_bytes_is_one_call():
    call = Stub(0)
    text = sized(call, None)
    assert call.calls == [(None, 0)]
    assert text.dtype == torch.uint8 and text.numel() == 0 and text.device == CPU


def test_sized_text_is_a_size_query_and_a_fill_of_exactly_total():
    call = Stub(5)
    text = sized(call, None)
    assert len(call.calls) == 2 and call.calls[0] == (None, 0)
    buf, cap = call.calls[1]
    assert buf is text and cap == 5
    assert text.dtype == torch.uint8 and text.numel() == 5 and text.is_contiguous()


def test_sized_text_into_out_is_one_call_and_a_view():
    call = Stub(5)
    out = torch.zeros(8, dtype=torch.uint8)
    text = sized(call, out)
    assert len(call.calls) == 1 and call.calls[0][0] is out and call.calls[0][1] == 8
    assert text.numel() == 5 and text.data_ptr() == out.data_ptr()


def test_sized_text_into_a_small_out_is_refused():
    call = Stub(5)
    with pytest.raises(api.RejitError) as e:
        sized(call, torch.zeros(4, dtype=torch.uint8))
    assert e.value.status == -4 and len(call.calls) == 1 and call.calls[0][1] == 4
    assert e.value.message == "pack_records: the packed text has 5 bytes, `out` 4"


def test_sized_text_into_an_empty_out_passes_no_buffer():
    call = Stub(0)
    text = sized(call, torch.zeros(0, dtype=torch.uint8))
    assert call.calls == [(None, 0)] and text.numel() == 0
    with pytest.raises(AssertionError):
        sized(Stub(0), torch.zeros(4, dtype=torch.int8))


def test_one_byte_argument():
    assert api._one_byte(44, "csv_records", "delimiter") == 44
    assert api._one_byte(b",", "csv_records", "delimiter") == 44
    with pytest.raises(ValueError) as e:
        api._one_byte(b",,", "csv_records", "delimiter")
    assert str(e.value) == "csv_records: delimiter is not one byte"
