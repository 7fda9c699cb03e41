"""The altcorr backward (training) surface without a GPU: the library exports, the HIP-only and dtype refusals."""
import pytest
import torch


def test_library_exports_the_backward_entry_points():
    from cdv_slam_amd import _lib
    lib = _lib.load()
    for n in ("cdv_corr_bwd", "cdv_patchify_bwd", "cdv_corr_bwd_workspace_bytes", "cdv_patchify_bwd_workspace_bytes"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    # the workspace depends on the shapes only, and grows with the edges
    a = lib.cdv_corr_bwd_workspace_bytes(1000, 100, 8, 3, 30, 40, 3)
    assert a > 0 and lib.cdv_corr_bwd_workspace_bytes(2000, 100, 8, 3, 30, 40, 3) > a
    assert lib.cdv_patchify_bwd_workspace_bytes(1, 80, 120, 160, 1) > 80 * 4


def test_backward_argument_errors_are_codes():
    from cdv_slam_amd import _lib
    lib = _lib.load()
    assert lib.cdv_corr_bwd(None, None, None, None, None, None, None, None, None, 10, 1, 1, 24, 3, 8, 8, 3, None) == -2
    assert lib.cdv_patchify_bwd(None, None, None, None, 1, 10, 8, 8, 8, 1, 2, None) == -4


def _corr_args(dtype):
    f1 = torch.zeros(1, 4, 8, 3, 3, dtype=dtype)
    f2 = torch.zeros(1, 2, 8, 10, 12, dtype=dtype)
    coords = torch.zeros(1, 5, 2, 3, 3)
    ii, jj = torch.zeros(5, dtype=torch.long), torch.zeros(5, dtype=torch.long)
    grad = torch.zeros(1, 5, 7, 7, 3, 3)
    return f1, f2, coords, ii, jj, grad, 3


def test_cuda_corr_backward_refuses_cpu_tensors():
    """the HIP-only refusal (RuntimeError), not a missing backward (NotImplementedError, itself a RuntimeError)"""
    from cdv_slam_amd.dropin import cuda_corr
    with pytest.raises(RuntimeError) as e:
        cuda_corr.backward(*_corr_args(torch.float32))
    assert not isinstance(e.value, NotImplementedError)
    net = torch.zeros(1, 8, 10, 12)
    with pytest.raises(RuntimeError) as e:
        cuda_corr.patchify_backward(net, torch.zeros(1, 5, 2), torch.zeros(1, 5, 8, 4, 4), 1)
    assert not isinstance(e.value, NotImplementedError)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_cuda_corr_backward_is_float32_only(dtype):
    """the reference's backward reads the window gradient as float: other map dtypes are a TypeError, checked before
    the device"""
    from cdv_slam_amd.dropin import cuda_corr
    with pytest.raises(TypeError, match="float32"):
        cuda_corr.backward(*_corr_args(dtype))
