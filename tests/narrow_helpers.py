"""Helpers shared by the GPU tests of the narrow kernels (test_narrow_gpu.py, test_narrow_mfma_gpu.py, test_narrow_rows_gpu.py and the later test_narrow*_gpu.py; the
seeded fuzzers of test_fuzz_narrow_gpu.py): one kn_spmm on a column window with its plan, and the recorder of the kn_spmm calls a forward issues."""
import torch

from keynet_amd import _capi

SENTINEL = 7.5


def _spmm(op, xd, n, flags, ld=None, start=0, absmax=None):
    """kn_spmm on columns start .. start + n of the contiguous block xd [cols, ldx] into the same window of a sentinel-filled block with ldy = ld (None: compact):
    (the window as a tensor, the whole y block, the plan)."""
    (rows, _) = op.shape()
    ldx = int(xd.shape[1])
    ldy = n if ld is None else ld
    y = torch.full((rows, ldy), SENTINEL, dtype=torch.float32, device=xd.device)
    with torch.cuda.device(xd.device):
        op.spmm(xd.data_ptr() + 4 * start, ldx, n, y.data_ptr() + 4 * start, ldy, flags, torch.cuda.current_stream().cuda_stream,
                absmax_ptr=None if absmax is None else absmax.data_ptr())
        plan = op.plan(n, flags, ldx=ldx, ldy=ldy)
    return (y[:, start:start + n], y, plan)


def _spmm_calls(monkeypatch):
    """Records (plan of the call, flags) of every kn_spmm / kn_spmm_screen the Python host issues from here on: the path a forward really takes."""
    calls = []
    spmm = _capi.Operator.spmm

    def recording(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr=None):
        calls.append((self.plan(n_vecs, flags, ldx=ldx, ldy=ldy), int(flags)))
        return spmm(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr)
    monkeypatch.setattr(_capi.Operator, 'spmm', recording)
    return calls
