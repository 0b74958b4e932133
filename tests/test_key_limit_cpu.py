"""block_sparse's one key-limit resolver (_check_limit) on the host forms of kv_len / start: every public call of the module
resolves its limits through it.  The device forms are pinned on the GPU by the "not read on the host" tests of each call."""
import pytest
import torch

from rectified_spaattn_amd.block_sparse import _check_limit

B, SK = 3, 700


@pytest.mark.parametrize("val,want", [
    (None, [SK, SK, SK]),
    (0, [0, 0, 0]),
    (333, [333, 333, 333]),
    (SK, [SK, SK, SK]),
    ([700, 0, 333], [700, 0, 333]),
    ((5, 6, 7), [5, 6, 7]),
    ([41], [41, 41, 41]),
    (torch.tensor([700, 0, 333]), [700, 0, 333]),
    (torch.tensor([[1], [2], [3]], dtype=torch.int32), [1, 2, 3]),
    (torch.tensor(9), [9, 9, 9]),
    (torch.tensor([2.0, 3.0, 4.0]), [2, 3, 4]),
], ids=["none", "zero", "int", "int-Sk", "list", "tuple", "list-of-1", "tensor", "tensor-2d", "tensor-0d", "tensor-float"])
def test_host_forms_become_one_int_per_batch_item(val, want):
    got = _check_limit("kv_len", val, B, SK, SK)
    assert got == want and all(type(n) is int for n in got)
    assert _check_limit("kv_len", val, B, SK, SK, device_ok=False) == want      # (the call without a device form: the same)


def test_the_default_is_the_callers():
    assert _check_limit("start", None, 2, SK, 0) == [0, 0]
    assert _check_limit("kv_len", None, 2, SK, SK) == [SK, SK]


@pytest.mark.parametrize("name", ["kv_len", "start"])
@pytest.mark.parametrize("val,what", [(SK + 1, "outside"), (-1, "outside"), ([1, 2, SK + 1], "outside"), (torch.tensor([-1, 0, 0]), "outside"),
                                      ([1, 2], "2 values for a batch of 3"), ([1, 2, 3, 4], "4 values for a batch of 3"),
                                      (torch.zeros(2, dtype=torch.int64), "2 values for a batch of 3"), ([], "0 values")])
def test_refusals_name_the_argument(name, val, what):
    with pytest.raises(ValueError, match=what) as e:
        _check_limit(name, val, B, SK, 0)
    assert str(e.value).startswith(name) and ("start" in str(e.value)) == (name == "start")
