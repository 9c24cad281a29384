"""The marshalling rules of api.py without a GPU and without a Context: the module-level halves.

  * check_tensor refuses whatever is no tensor of the dtype on the device with TypeError, naming the argument and the device;
  * cells_of, the numpy half of the cells path, is fr_cell row by row and refuses arrays that are no cells with ValueError;
  * argument_shape at both ends of k and n_sets."""
import numpy as np
import pytest

DEVICE = 3  # a fixed index: nothing here touches a device

NOT_TENSORS = {
    "a list": lambda torch, dtype: [1, 2, 3],
    "None": lambda torch, dtype: None,
    "a numpy array": lambda torch, dtype: np.zeros(4, dtype),
    "a CPU tensor of the right dtype": lambda torch, dtype: torch.zeros(4, dtype=getattr(torch, dtype)),
    "a CPU tensor of the wrong dtype": lambda torch, dtype: torch.zeros(4, dtype=torch.int64),
}


@pytest.mark.parametrize("dtype", ["uint8", "int32"])
@pytest.mark.parametrize("what", sorted(NOT_TENSORS))
def test_check_tensor_refuses_what_is_no_device_tensor_of_the_dtype(pkg, what, dtype):
    import torch
    value = NOT_TENSORS[what](torch, dtype)
    for kwargs in ({}, {"shape": (4,)}, {"min_bytes": 1}, {"nbytes": 4}):
        with pytest.raises(TypeError) as e:
            pkg.api.check_tensor(value, "the_argument", DEVICE, dtype, **kwargs)
        assert "the_argument" in str(e.value) and "cuda:%d" % DEVICE in str(e.value) and dtype in str(e.value)


def test_check_tensor_says_what_else_the_caller_takes(pkg):
    with pytest.raises(TypeError, match="mapping .*cuda:3, or a numpy array"):
        pkg.api.check_tensor(None, "mapping", DEVICE, "int32", alt=", or a numpy array")


R_MINUS_1 = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000
VALUES = [0, 1, 7, R_MINUS_1]


def test_cells_of_is_fr_cell_row_by_row(pkg):
    api = pkg.api
    r = api.FR_MODULUS
    assert R_MINUS_1 == r - 1
    for v in VALUES:
        assert api.cells_of(v).tobytes() == api.fr_cell(v).tobytes() and api.cells_of(v).shape == (1, 32)
    assert api.cells_of(np.int64(7)).tobytes() == api.fr_cell(7).tobytes()
    assert api.cells_of(np.uint32(7)).tobytes() == api.fr_cell(7).tobytes()
    seq = api.cells_of(VALUES)
    assert seq.shape == (len(VALUES), 32) and seq.dtype == np.uint8
    assert seq.tobytes() == b"".join(api.fr_cell(v).tobytes() for v in VALUES)
    assert api.cells_of(tuple(VALUES)).tobytes() == seq.tobytes()
    # a value of r or more is reduced, a negative one too
    assert api.cells_of(r + 5).tobytes() == api.fr_cell(5).tobytes()
    assert api.cells_of([r, 2 * r + 1, -1]).tobytes() == api.cells_of([0, 1, r - 1]).tobytes()
    # cells as numpy are taken as they lie
    assert api.cells_of(seq) is seq
    assert api.cells_of(seq[0]).shape == (32,)


def test_cells_of_refuses_arrays_that_are_no_cells(pkg):
    for bad in (np.zeros((2, 32), np.int32), np.zeros((2, 31), np.uint8), np.zeros(31, np.uint8), np.zeros((), np.uint8),
                np.zeros((2, 32), np.float32)):
        with pytest.raises(ValueError, match="points"):
            pkg.api.cells_of(bad, "points")
    for bad in (None, 1.5, object(), [None]):
        with pytest.raises(TypeError, match="points"):
            pkg.api.cells_of(bad, "points")


@pytest.mark.parametrize("k, n_sets, shape", [
    (10, 1, (1, 5, 1024)), (30, 1024, (1024, 5, 1 << 30)), (31, 1, (0,)), (10, 0, (0,)), (10, 1025, (0,)),
    (0, 1, (1, 5, 1)), (-1, 1, (0,)), (10, -1, (0,))])
def test_argument_shape(pkg, k, n_sets, shape):
    assert pkg.api.argument_shape(k, n_sets) == shape


def test_table_shapes(pkg):
    assert pkg.api.TABLE_FR_SHAPE == (3, pkg.TABLE_ROWS, 32) and pkg.api.INV_FR_SHAPE == (2, 3, pkg.TABLE_ROWS, 32)
    assert pkg.TABLE_ROWS == 66561
