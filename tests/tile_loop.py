"""What tests/test_gpu_tile_loop.py and tests/test_tile_loop_cpu.py share: the tile sizes of the six persistent chain
kernels (csrc/chain_tile.h), the batch sizes that make a workgroup walk past its first tile, and the float64 (or
float32) evaluation on the CPU of everything those kernels write -- the per-row buffers included.  No test lives here.
"""
import torch
import torch.nn.functional as F

from oracle import detrand
from oracle import mlp as omlp

W0 = 30.0
GRID_BLOCKS = 256  # chain_blocks / mod_blocks / kGradMaxBlocks / kMaxBlocks: at most 256 workgroups walk the tiles

# R, the rows (gradient kernels: points) of a tile, per kernel family and hidden width.  One table: a stale entry makes
# the GPU tests stop wrapping without failing, so test_tile_loop_cpu.py holds the SIREN rows to the library.
SIREN_ROWS = {256: 64, 128: 128, 64: 256, 32: 256}     # siren_chain.hip tile_rows() = Shape<H>::rows = 32 RB, CT = 64
MOD_ROWS = {128: 64, 64: 128}                          # modsiren.hip mod_tile_rows() = MShape<H>::rows, CT = 32
SIREN_GRAD_POINTS = {256: 16, 128: 32, 64: 64, 32: 64}  # siren_gradient.hip GradShape<H, 4>::points = rows / 4 (mri_inr.h:
SIREN_GRAD4_POINTS = {256: 8, 128: 16, 64: 32, 32: 32}  # "1024 / hidden, 64 at hidden 32"); GradShape<H, 8>: "half as many"
MOD_GRAD_POINTS = {128: 16, 64: 32}                    # modsiren_gradient.hip MGradShape<H>::points ("2048 / hidden")


def siren_grad_points(hidden, dim_in):
    return (SIREN_GRAD4_POINTS if dim_in == 4 else SIREN_GRAD_POINTS)[hidden]


# With T = 256 R:
#   T            every workgroup has exactly one full tile: nobody may prefetch weights for a next tile
#   T + 1        workgroup 0 alone has a second tile, of one row; the other 255 take "no next tile" in the same launch
#   T + R + 3    workgroups 0 and 1 have a second tile, workgroup 1's is ragged (3 rows)
#   2 T + R + 3  every workgroup has two full tiles, workgroup 0 a third full one, workgroup 1 a third of 3 rows
SIZE_NAMES = ("T", "T+1", "T+R+3", "2T+R+3")


def batch_sizes(rows):
    t = GRID_BLOCKS * rows
    return dict(zip(SIZE_NAMES, (t, t + 1, t + rows + 3, 2 * t + rows + 3)))


def uniform(n, cols, seed):
    return torch.from_numpy(detrand.uniform(n * cols, seed, -1.0, 1.0).reshape(n, cols).copy())


def intensities(n, seed):
    """Targets in [0, 1], as image intensities are.  The head's bias gradient is the single number 2 mean(y - target).
    Against zero-mean targets that have nothing to do with the network it is a chance cancellation of about
    1.2 / sqrt(n), and where chance makes it a hundred times smaller no float32 evaluation is within REL_TOL of it: at
    3 -> 128 x 3, n = 32768, targets in [-1, 1], it is 5.0e-5 (6.6e-3 is typical), and the float32 terms 2 (y - t) / n of
    torch's CPU forward summed EXACTLY are 1.7e-5 of it away -- the rounding of y alone.  Against intensities the
    untrained network's y - target averages about -0.5 and the number is as well conditioned as the other gradients."""
    return torch.from_numpy(detrand.uniform(n, seed, 0.0, 1.0).reshape(n, 1).copy())


# ------------------------------------------------------------------------------------------------ SIREN chain, float64
def siren_float64(params, x, target, tail_from):
    """SirenNet + F.mse_loss in float64 on the float32 inputs, with everything the chain kernels write: y, the loss, per
    sine layer act = sin(w0 z_l) and deriv = w0 cos(w0 z_l) (z_l the layer's linear output), dz[l] = dLoss / dz_l for
    l >= 1, every parameter gradient in (w, b) order -- and the loss and gradients of the rows >= tail_from alone
    (loss_tail = sum over those rows of (y - target)^2 / n: what is left when dLoss/dy of the other rows is zero)."""
    n = x.shape[0]
    ps = [(w.double().requires_grad_(True), b.double().requires_grad_(True)) for w, b in params]
    flat = [t for wb in ps for t in wb]
    h, z = x.double(), []
    for w, b in ps[:-1]:
        z.append(F.linear(h, w, b))
        h = torch.sin(W0 * z[-1])
    y = F.linear(h, *ps[-1])
    with torch.no_grad():
        assert torch.equal(y, omlp.siren_forward(x.double(), ps, w0=W0, w0_initial=W0)), "not the oracle's forward"
    sq = (y - target.double().reshape(-1, 1)) ** 2
    loss, loss_tail = sq.sum() / n, sq[tail_from:].sum() / n
    g = torch.autograd.grad(loss, flat + z[1:], retain_graph=True)
    out = dict(y=y.detach(), loss=float(loss), grads=list(g[:len(flat)]), dz=[None] + list(g[len(flat):]),
               act=[torch.sin(W0 * v).detach() for v in z], deriv=[(W0 * torch.cos(W0 * v)).detach() for v in z],
               loss_tail=float(loss_tail))
    out["grads_tail"] = list(torch.autograd.grad(loss_tail, flat)) if tail_from < n else None
    return out


# ------------------------------------------------------------------------------------------------ modulated chain
def mod_reference(ref, x, target, tail_from):
    """ModulatedSirenNet + F.mse_loss by the formulas of test_gpu_modsiren.ModRef `ref`, in its dtype, with everything
    the modulated chain kernels write: per layer act = s (.) h, hid = h = relu(pm), dcos = h (.) w0 cos(w0 ps), sn = s =
    sin(w0 ps) (ps, pm: the two stacks' linear outputs), dzs[l] = dLoss / dps_l and dzm[l] = dLoss / dpm_l for l >= 1,
    the gradients in the order of ModRef.parameters(), and loss / gradients of the rows >= tail_from alone."""
    dt, n = ref.dtype, x.shape[0]
    z = x.to(dt)
    a, hm, ps, pm = z, z, [], []
    saved = dict(act=[], hid=[], dcos=[], sn=[])
    for (ws, bs), (wm, bm) in zip(ref.siren[:-1], ref.mod):
        ps.append(F.linear(a, ws, bs))
        pm.append(F.linear(hm, wm, bm))
        s, h = torch.sin(W0 * ps[-1]), torch.relu(pm[-1])
        a, hm = s * h, torch.cat((h, z), dim=1)
        for k, v in zip(("act", "hid", "dcos", "sn"), (a, h, h * (W0 * torch.cos(W0 * ps[-1])), s)):
            saved[k].append(v.detach())
    y = F.linear(a, *ref.siren[-1])
    with torch.no_grad():
        assert torch.equal(y, omlp.modulated_siren_forward(z, ref.siren, ref.mod, W0, W0)), "not the oracle's forward"
    sq = (y - target.to(dt).reshape(-1, 1)) ** 2
    loss, loss_tail = sq.sum() / n, sq[tail_from:].sum() / n
    flat, k = ref.parameters(), len(ps) - 1
    g = torch.autograd.grad(loss, flat + ps[1:] + pm[1:], retain_graph=True)
    out = dict(saved, y=y.detach(), loss=float(loss), grads=list(g[:len(flat)]),
               dzs=[None] + list(g[len(flat):len(flat) + k]), dzm=[None] + list(g[len(flat) + k:]),
               loss_tail=float(loss_tail))
    out["grads_tail"] = list(torch.autograd.grad(loss_tail, flat)) if tail_from < n else None
    return out
