"""igm_population_transpose on the MI355X: both directions of the move between the A-step layout
(nbead, nstruct, 3) and the M-step layout (nstruct, natom, 3), bit for bit against a NumPy
transpose, on tile-edge shapes, through host arrays and through device pointers."""
import numpy as np
import pytest

from igm_amd._lib import IGM_DEVICE_PTRS, IGM_E_INVALID, IGM_OK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from igm_amd import _lib
    return _lib.context(0)


SHAPES = [(1, 1, 1), (31, 33, 31), (32, 32, 40), (33, 31, 36), (100, 70, 103), (257, 5, 260)]


def distinct(shape, base):
    """float32 array with a different value in every element (integers below 2**24)"""
    n = int(np.prod(shape))
    assert base + n < 2 ** 24
    return (base + np.random.default_rng(n).permutation(n)).astype(np.float32).reshape(shape)


def transpose(ctx, nbead, S, natom, src, dst, direction, device):
    if not device:
        return ctx.lib.igm_population_transpose(ctx.h, 0, nbead, S, natom, src.ctypes.data, dst.ctypes.data, direction)
    import torch
    tsrc, tdst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        rc = ctx.lib.igm_population_transpose(ctx.h, IGM_DEVICE_PTRS, nbead, S, natom, tsrc.data_ptr(),
                                              tdst.data_ptr(), direction)
    finally:
        ctx.set_stream(None)
    torch.cuda.synchronize()
    dst[...] = tdst.cpu().numpy()
    assert tsrc.cpu().numpy().tobytes() == src.tobytes()  # the source is only read
    return rc


@pytest.mark.parametrize('device', [False, True])
@pytest.mark.parametrize('nbead,S,natom', SHAPES)
def test_gpu_population_transpose(ctx, nbead, S, natom, device):
    """both directions bit-equal to a NumPy transpose; direction 0 leaves the atoms past nbead as
    the caller had them, direction 1 does not read them; the round trip restores the source"""
    bm = distinct((nbead, S, 3), 1)
    sm = distinct((S, natom, 3), 5000000)  # no value in common with bm
    # direction 0: bead-major -> struct-major
    out = sm.copy()
    assert transpose(ctx, nbead, S, natom, bm, out, 0, device) == IGM_OK
    assert out[:, :nbead].tobytes() == np.ascontiguousarray(bm.transpose(1, 0, 2)).tobytes()
    assert out[:, nbead:].tobytes() == sm[:, nbead:].tobytes()
    # direction 1: struct-major -> bead-major, the extra atoms are not part of the result
    back = np.full((nbead, S, 3), -1.0, np.float32)
    assert transpose(ctx, nbead, S, natom, out, back, 1, device) == IGM_OK
    assert back.tobytes() == bm.tobytes()  # round trip
    src = sm.copy()
    src[:, nbead:] = np.nan
    res = np.full((nbead, S, 3), -1.0, np.float32)
    assert transpose(ctx, nbead, S, natom, src, res, 1, device) == IGM_OK
    assert res.tobytes() == np.ascontiguousarray(sm[:, :nbead].transpose(1, 0, 2)).tobytes()


@pytest.mark.parametrize('nbead,S,natom,direction', [(5, 3, 4, 0), (5, 3, 4, 1), (5, 3, 6, 2), (5, 3, 6, -1),
                                                     (0, 3, 6, 0), (5, 0, 6, 1)])
def test_gpu_population_transpose_invalid_arguments(ctx, nbead, S, natom, direction):
    src = np.zeros(200, np.float32)
    dst = np.full(200, 3.0, np.float32)
    rc = ctx.lib.igm_population_transpose(ctx.h, 0, nbead, S, natom, src.ctypes.data, dst.ctypes.data, direction)
    assert rc == IGM_E_INVALID
    assert np.all(dst == 3.0)
