"""Host-side checks of the training up-sampling entries (no device needed): the two ABI names, their argument errors
before any launch, and the `channels` keyword of RAFTStereo.upsample_flow on the CPU path."""
import ctypes

import torch

import _upsample_ref as R


def test_entries_refuse_bad_arguments_before_launch():
    from dkt_stereo_amd import _ffi
    lib = _ffi.lib()
    fwd, bwd = lib.dkt_convex_upsample_fwd, lib.dkt_convex_upsample_bwd
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    base += -base % 16                                               # a 16-byte aligned address inside the buffer
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    assert fwd(null, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert fwd(p, p, null, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert fwd(p, p, p, 1, 0, 1, 2, 2, 4, -1, null) == -2            # D = 0
    assert fwd(p, p, p, 1, 2, 0, 2, 2, 4, -1, null) == -2            # Dout = 0
    assert fwd(p, p, p, 1, 2, 3, 2, 2, 4, -1, null) == -2            # Dout > D
    assert fwd(p, p, p, 1, 2, 1, 2, 2, 0, -1, null) == -2            # factor = 0
    assert fwd(p, p, p, 1, 2, 1, 2, 2, 16, -1, null) == -7           # factor beyond 8
    assert fwd(p, p, p, 65536, 2, 1, 2, 2, 4, -1, null) == -7        # N beyond the grid
    assert fwd(p, p, off, 1, 2, 1, 2, 2, 4, -1, null) == -6          # out rows are stored 16 bytes at a time
    assert bwd(null, 64, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -1
    assert bwd(p, 64, p, p, null, null, p, 1, 2, 1, 2, 2, 4, -1, null) == -1     # neither gradient wanted
    assert bwd(p, 64, p, p, p, p, null, 1, 2, 1, 2, 2, 4, -1, null) == -1        # gflow needs the workspace
    assert bwd(p, 63, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -2           # batch stride shorter than an image
    assert bwd(p, 66, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -6           # batch stride not a multiple of f
    assert bwd(off, 64, p, p, p, p, p, 1, 2, 1, 2, 2, 4, -1, null) == -6
    assert bwd(p, 64, p, p, p, p, p, 1, 2, 1, 2, 2, 3, -1, null) == -7


def test_upsample_flow_channels_on_the_cpu_path():
    """CPU tensors take the reference's expression sequence; channels = c is its leading c channels, with a gradient."""
    from dkt_stereo_amd.raft_stereo import RAFTStereo, make_args
    model = RAFTStereo(make_args())
    flow, mask, _, f, _ = R.inputs(R.CASES["f4"])
    a = torch.from_numpy(flow).requires_grad_(True)
    b = torch.from_numpy(mask).requires_grad_(True)
    full = model.upsample_flow(a, b)
    assert torch.equal(full, R.sequence(a, b, f))
    one = model.upsample_flow(a, b, channels=1)
    assert one.shape[1] == 1 and torch.equal(one, full[:, :1])
    ga, gb = torch.autograd.grad(one.sum(), (a, b))
    wa, wb = torch.autograd.grad(full[:, :1].sum(), (a, b))
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
