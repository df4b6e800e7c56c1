"""torch.autograd glue around the C ABI of libnnr.so.

`render_rays` is the one differentiable operator the host-side `model.Renderer` calls: sampling along rays,
the positional-encoded MLP and alpha-compositing, forward and backward, entirely in the HIP kernels
(reference model/rendering.py:95-132 + model/official_nerf.py:60-96 and autograd through them).
PyTorch is used for device memory, the current stream and the autograd graph edge -- nothing is computed here.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import logging
import threading
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import lib as L


def _require_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("nnr: the render path runs only on an AMD GPU (HIP); got a CPU tensor and there is no CPU fallback")
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        # the kernels are launched on the current device's current stream (one process per GPU: torch.cuda.set_device(local_rank))
        raise RuntimeError("nnr: tensors live on cuda:%d but the current device is cuda:%d; call torch.cuda.set_device first"
                           % (t.device.index, torch.cuda.current_device()))


# ----------------------------------------------------------------------------------------------------------------------
# packed weights: re-packed only when a parameter tensor changed (optimizer.step bumps tensor._version)
# ----------------------------------------------------------------------------------------------------------------------
_param_epoch = 0   # bumped after every torch optimizer step, see _after_any_optimizer_step


def _after_any_optimizer_step(optimizer, args, kwargs):
    """Global optimizer post-step hook.  tensor._version is NOT a reliable change detector: torch's fused optimizers
    (Adam(fused=True) -- which model.Trainer selects) update parameters in place without bumping it, and a stale packed
    copy means the render kernels silently keep using old weights.  Any optimizer step therefore invalidates every pack."""
    global _param_epoch
    _param_epoch += 1


from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook  # noqa: E402

_register_step_hook(_after_any_optimizer_step)


def invalidate_packed_weights():
    """For code that changes parameters behind torch's back (custom kernels writing through .data_ptr())."""
    global _param_epoch
    _param_epoch += 1


class _PackCache:
    """Valid only for the very same tensor objects (weak references -- a data_ptr or id() can be recycled by a new model
    after the old one is freed) at the very same in-place versions, with no optimizer step since."""

    def __init__(self, hidden, tensors, packed):
        self.hidden = hidden   # (width, bf16 mode): the two modes have different packed layouts
        self.refs = [weakref.ref(t) for t in tensors]
        self.versions = [t._version for t in tensors]
        self.epoch = _param_epoch
        self.packed = packed

    def matches(self, hidden, tensors):
        return (self.hidden == hidden and self.epoch == _param_epoch and len(self.refs) == len(tensors)
                and all(r() is t for r, t in zip(self.refs, tensors))
                and self.versions == [t._version for t in tensors])


_pack_caches = {}   # id(first weight) -> _PackCache; a handful of live models at most


def _packed_for(cfg, weights, biases):
    """Packed (MFMA-fragment order) copy of the 24 parameter tensors; `weights`/`biases` must be the caller's long-lived
    tensor objects (nn.Parameters), not temporaries."""
    tensors = [*weights, *biases]
    mode = (cfg.hidden, cfg.flags & (L.NNR_F_BF16 | L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2))     # each product mode has its own packed layout
    key = (id(tensors[0]), mode[1])
    hit = _pack_caches.get(key)
    if hit is not None and hit.matches(mode, tensors):
        return hit.packed
    lib = L.load()
    n = lib.nnr_packed_floats(C.byref(cfg))
    packed = torch.empty(n, dtype=torch.float32, device=tensors[0].device)
    ps = L.params_struct([w.detach() for w in weights], [b.detach() for b in biases])
    L.check(lib.nnr_pack_weights(C.byref(cfg), C.byref(ps), L.ptr(packed),
                                 L.stream()), "nnr_pack_weights")
    for k in [k for k, v in _pack_caches.items() if any(r() is None for r in v.refs)]:
        del _pack_caches[k]             # drop entries of models that no longer exist
    _pack_caches[key] = _PackCache(mode, tensors, packed)
    return packed


# ----------------------------------------------------------------------------------------------------------------------
# workspaces and plans, cached per (device, shape); a training workspace is held by the autograd node until backward
# ----------------------------------------------------------------------------------------------------------------------
_ws_pool = {}
_plan_cache = {}


def _cfg_key(cfg: L.Cfg, device):
    return (str(device), cfg.n_rays, cfg.n_samples, cfg.hidden, cfg.flags)


_WS_SIZER = {None: "nnr_workspace_floats", "frozen": "nnr_frozen_workspace_floats", "frozen_sparse": "nnr_frozen_sparse_workspace_floats"}


def _ws_pool_of(cfg: L.Cfg, device, kind):
    return _ws_pool.setdefault(_cfg_key(cfg, device) + ((kind,) if kind else ()), [])


def _take_workspace(cfg: L.Cfg, device, kind=None) -> torch.Tensor:
    """kind: None, the workspace of include/nnr.h; "frozen", the frozen-field workspace of include/nnr_frozen.h (the same cfg, a far smaller
    buffer); "frozen_sparse", the one of include/nnr_frozen_sparse.h (the same planes and the live list behind them).  A pool per kind."""
    pool = _ws_pool_of(cfg, device, kind)
    if pool:
        return pool.pop()
    n = getattr(L.load(), _WS_SIZER[kind])(C.byref(cfg))
    if n == 0:
        raise RuntimeError("nnr: unsupported configuration (hidden_dim must be 128 or 256; num_points <= 1024 for training)")
    return torch.empty(n, dtype=torch.float32, device=device)


def _give_workspace(cfg: L.Cfg, device, ws: torch.Tensor, kind=None):
    pool = _ws_pool_of(cfg, device, kind)
    if len(pool) < 2:
        pool.append(ws)


def _plan_blob(cfg: L.Cfg) -> bytes:
    """The weight-gradient plan of cfg as nnr_plan_build writes it (include/nnr.h), on the host."""
    lib = L.load()
    raw = C.create_string_buffer(lib.nnr_plan_bytes(C.byref(cfg)))
    L.check(lib.nnr_plan_build(C.byref(cfg), C.cast(raw, C.c_void_p)), "nnr_plan_build")
    return raw.raw


def _plan_counts(cfg: L.Cfg):
    nj, nw = C.c_int32(0), C.c_int32(0)
    L.check(L.load().nnr_plan_counts(C.byref(cfg), C.byref(nj), C.byref(nw)), "nnr_plan_counts")
    return nj.value, nw.value


def _plan_for(cfg: L.Cfg, device) -> torch.Tensor:
    key = _cfg_key(cfg, device)
    plan = _plan_cache.get(key)
    if plan is None:
        plan = torch.from_numpy(np.frombuffer(_plan_blob(cfg), dtype=np.uint8).copy()).to(device)
        _plan_cache[key] = plan
    return plan


def plan_jobs(cfg: L.Cfg, with_waves: bool = False):
    """Host copy of the weight-gradient plan as a list of WgradJob (for tests / DESIGN inspection); with_waves also
    returns the wave_first table (wave w runs jobs [wave_first[w], wave_first[w+1]))."""
    (nj, nw), raw = _plan_counts(cfg), _plan_blob(cfg)
    assert len(raw) >= nj * C.sizeof(L.WgradJob) + 4 * (nw + 1 + 1)      # + n_heads and the head list (split 0 of every tile)
    jobs = list((L.WgradJob * nj).from_buffer_copy(raw, 0))
    if not with_waves:
        return jobs
    first = list((C.c_int32 * (nw + 1)).from_buffer_copy(raw, nj * C.sizeof(L.WgradJob)))
    return jobs, first


def plan_bf16(cfg: L.Cfg):
    """Host copy of the bf16-mode weight-gradient plan: (jobs, block_first, outputs) -- for tests / DESIGN inspection."""
    (nj, nw), raw = _plan_counts(cfg), _plan_blob(cfg)
    n_blocks = nw // 4
    o1 = nj * C.sizeof(L.WgradJobB)
    o2 = o1 + 4 * (n_blocks + 1)
    n_out = (len(raw) - o2) // C.sizeof(L.WgradOutB)
    assert o2 + n_out * C.sizeof(L.WgradOutB) == len(raw)
    jobs = list((L.WgradJobB * nj).from_buffer_copy(raw, 0))
    first = list((C.c_int32 * (n_blocks + 1)).from_buffer_copy(raw, o1))
    outs = list((L.WgradOutB * n_out).from_buffer_copy(raw, o2))
    return jobs, first, outs


def workspace_plane(cfg: L.Cfg, ws: torch.Tensor, plane: int, n_rows: Optional[int] = None) -> torch.Tensor:
    """One workspace plane as (rows, width) -- used by the parity tests to localise a mismatch.  A view for the fp32 planes; the
    planes a bf16 training workspace stores as tile-major bf16 (hidden activations 11..18, 20, the encodings' copies 21, 22 and the
    gradients 31..38, 40: nnr_layout.h) come back in natural [sample][feature] order, converted to fp32."""
    pitch = C.c_int32(0)
    off = L.load().nnr_ws_plane(C.byref(cfg), plane, C.byref(pitch))
    if off < 0:
        raise KeyError(plane)
    S = cfg.n_rays * cfg.n_samples
    rows = n_rows if n_rows is not None else S
    if L.load().nnr_ws_plane_layout(C.byref(cfg), plane) == 2:
        # tile-major fp32 (the gradient planes of a three-term training workspace): [chunk of 32 samples][octet j][half h][sample c][i],
        # feature = 8 j + 4 h + i  (nnr_layout.h: tile32_index); back in natural [sample][feature] order (a copy)
        W = pitch.value
        chunks = (rows + 31) // 32
        t = ws[off: off + chunks * 32 * W].view(chunks, W // 8, 2, 32, 4)                       # [chunk][j][h][c][i]
        return t.permute(0, 3, 1, 2, 4).reshape(chunks * 32, W)[:rows]                          # [chunk][c] x [j][h][i]
    stored_bf16 = (cfg.flags & L.NNR_F_BF16) and (cfg.flags & L.NNR_F_TRAIN) and (11 <= plane <= 18 or 20 <= plane <= 22 or 31 <= plane <= 38 or plane == 40)
    if not stored_bf16:
        return ws[off: off + rows * pitch.value].view(rows, pitch.value)
    # tile-major: [chunk of 32 samples][group of 16 features][half h][sample c][second quad j][i]; feature = 16 g + 4 h + 8 j + i
    G = pitch.value // 8
    chunks = (rows + 31) // 32
    t = ws[off: off + chunks * 32 * pitch.value].view(torch.bfloat16).view(chunks, G, 2, 32, 2, 4)    # [chunk][g][h][c][j][i]
    return t.permute(0, 3, 1, 4, 2, 5).reshape(chunks * 32, G * 16)[:rows].float()                    # [chunk][c] x [g][j][h][i]


# ----------------------------------------------------------------------------------------------------------------------
# the operator
# ----------------------------------------------------------------------------------------------------------------------
def _ray_inputs(rays, z_lo, z_hi, jitter):
    """What every render entry point reads of its rays: the (R,3) tensors `rays`, the two (N) z tables and the jitter -- (R,N), or None,
    which stays None -- detached, contiguous and fp32.  -> (list of rays, z_lo, z_hi, jitter)"""
    R, N = rays[0].shape[0], z_lo.shape[0]
    rays = [t.detach().contiguous().float() for t in rays]
    z_lo, z_hi = z_lo.detach().contiguous().float(), z_hi.detach().contiguous().float()
    return rays, z_lo, z_hi, (jitter.detach().contiguous().float().view(R, N) if jitter is not None else None)


class _RenderRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts_o, pts_d, view_d, z_lo, z_hi, jitter, opts, *params):
        weights, biases = params[:L.N_LAYERS], params[L.N_LAYERS:]
        _require_gpu(pts_o)
        dev = pts_o.device
        R, N = pts_o.shape[0], z_lo.shape[0]
        need_grad = any(ctx.needs_input_grad)
        cfg = L.make_cfg(R, N, opts["hidden"], dist_alpha=opts["dist_alpha"], white_bg=opts["white_bg"],
                         relu_sigma=opts["relu_sigma"], train=need_grad, bf16=opts.get("bf16", False))
        lib = L.load()
        f32 = dict(dtype=torch.float32, device=dev)
        (pts_o, pts_d, view_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d, view_d), z_lo, z_hi, jitter)
        packed = _packed_for(cfg, *opts["params"])
        ws = _take_workspace(cfg, dev)
        rgb = torch.empty(R, 3, **f32)
        dist = torch.empty(R, **f32)
        # forward-only callers that do not want the per-sample outputs (samples=False) get the fused path of nnr_render_fwd: the
        # compositing happens in the MLP kernel's epilogue and nothing per-sample is written to HBM
        want_samples = need_grad or opts.get("samples", True)
        alpha = torch.empty(R, N, **f32) if want_samples else None
        zv = torch.empty(R, N, **f32) if want_samples else None
        st = L.stream()
        L.check(lib.nnr_render_fwd(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(view_d), L.ptr(z_lo), L.ptr(z_hi),
                                   L.ptr(jit), L.ptr(packed), L.ptr(rgb), L.ptr(dist), L.ptr(alpha), L.ptr(zv), L.ptr(ws), st),
                "nnr_render_fwd")
        rd = opts.get("ray_distortion", None)
        dloss = None      # (stays None where nothing is to be differentiated: no launch, no fifth value)
        if rd is not None and need_grad:
            # the ray distortion of the weights (nnr_ray_distortion.hip), read off the kept workspace: sigma_raw is column 3 of plane 0, z plane 1
            dloss = torch.empty(R, **f32)
            L.check(lib.nnr_ray_distortion_fwd(C.byref(cfg), _ws_column(cfg, ws, 0, 3), 4, _ws_column(cfg, ws, 1, 0), rd[0], rd[1],
                                               L.ptr(dloss), st), "nnr_ray_distortion_fwd")
        if need_grad:
            ctx.cfg, ctx.ws, ctx.packed, ctx.dev = cfg, ws, packed, dev
            ctx.shapes = [tuple(p.shape) for p in params]
            ctx.ray_distortion = rd
        else:
            _give_workspace(cfg, dev, ws)
        if want_samples:
            ctx.mark_non_differentiable(alpha, zv)
        ctx.set_materialize_grads(False)      # undefined upstream gradients arrive as None, not as zero-filled tensors
        if rd is not None:
            return rgb, dist, alpha, zv, dloss
        return rgb, dist, alpha, zv

    @staticmethod
    def backward(ctx, d_rgb, d_dist, _da, _dz, d_dloss=None):
        cfg, ws, dev = ctx.cfg, ctx.ws, ctx.dev
        if ws is None:
            raise RuntimeError("nnr: backward called twice on the same render (workspace already released)")
        lib = L.load()
        R = cfg.n_rays
        f32 = dict(dtype=torch.float32, device=dev)
        d_rgb = (d_rgb if d_rgb is not None else torch.zeros(R, 3, **f32)).contiguous().float()
        d_dist = (d_dist if d_dist is not None else torch.zeros(R, **f32)).contiguous().float()
        st = L.stream()
        need_w = any(ctx.needs_input_grad[7:])
        need_rays = any(ctx.needs_input_grad[:3])
        L.check(lib.nnr_composite_bwd(C.byref(cfg), L.ptr(d_rgb), L.ptr(d_dist), L.ptr(ws), st), "nnr_composite_bwd")
        if d_dloss is not None:
            # the regulariser's d(sigma_raw) joins the compositor's in column 3 of plane 2, before the MLP's backward reads it
            rd = ctx.ray_distortion
            d_dloss = d_dloss.contiguous().float()
            L.check(lib.nnr_ray_distortion_bwd(C.byref(cfg), _ws_column(cfg, ws, 0, 3), 4, _ws_column(cfg, ws, 1, 0), rd[0], rd[1],
                                               L.ptr(d_dloss), _ws_column(cfg, ws, 2, 3), 4, 1, st), "nnr_ray_distortion_bwd")
        L.check(lib.nnr_mlp_dgrad(C.byref(cfg), L.ptr(ctx.packed), L.ptr(ws), st), "nnr_mlp_dgrad")
        grads: List[Optional[torch.Tensor]] = [None] * (2 * L.N_LAYERS)
        if need_w:
            sizes = [int(np.prod(s)) for s in ctx.shapes]
            offs = np.cumsum([0] + [(n + 3) // 4 * 4 for n in sizes])          # keep every view 16-byte aligned
            # ONE allocation for all 24 gradients (the weight-gradient stage overwrites every element: no zero-fill launch) + GRAD_TAIL spare
            # floats behind them: autograd adopts the views as the parameters' .grad, so under data parallelism the step's all-reduce runs
            # IN PLACE on this buffer, the handful of pose / distortion gradients and logged scalars riding in the tail (nnr/parallel.py)
            # Under data parallelism the buffer is all-reduced as it lies, alignment gaps and tail included: zero-filled then (a NaN left over in a
            # gap would be summed -- never read, but a NaN check on the collective would trip), and REGISTERED with its used length: the in-place
            # path of nnr/parallel.py is taken for a buffer this function made, not for any storage that happens to hold many gradients.
            from . import parallel as _par
            if _par.world_size() > 1 or _par.always_reduce():
                flat = torch.zeros(int(offs[-1]) + GRAD_TAIL, **f32)
                register_flat_grads(flat, int(offs[-1]))
            else:
                flat = torch.empty(int(offs[-1]) + GRAD_TAIL, **f32)
            views = [flat[offs[i]: offs[i] + sizes[i]].view(ctx.shapes[i]) for i in range(2 * L.N_LAYERS)]
            gs = L.params_struct(views[:L.N_LAYERS], views[L.N_LAYERS:])
            L.check(lib.nnr_mlp_wgrad(C.byref(cfg), L.ptr(ctx.packed), C.byref(gs), L.ptr(_plan_for(cfg, dev)), L.ptr(ws), st), "nnr_mlp_wgrad")
            grads = [v if ctx.needs_input_grad[7 + i] else None for i, v in enumerate(views)]
        d_o = d_d = d_v = None
        if need_rays:
            d_o, d_d, d_v = (torch.empty(R, 3, **f32) for _ in range(3))
            L.check(lib.nnr_ray_reduce(C.byref(cfg), L.ptr(d_o), L.ptr(d_d), L.ptr(d_v), L.ptr(ws), st), "nnr_ray_reduce")
        ctx.ws = None
        _give_workspace(cfg, dev, ws)
        return (d_o, d_d, d_v, None, None, None, None, *grads)


def _ws_column(cfg: L.Cfg, ws: torch.Tensor, plane: int, col: int):
    """Device pointer of column `col` of a row-major fp32 workspace plane (nnr_ws_plane's offset)."""
    pitch = C.c_int32(0)
    off = L.load().nnr_ws_plane(C.byref(cfg), plane, C.byref(pitch))
    if off < 0 or col >= pitch.value or L.load().nnr_ws_plane_layout(C.byref(cfg), plane) != 0:
        raise RuntimeError("nnr: workspace plane %d has no row-major column %d" % (plane, col))
    return C.c_void_p(ws.data_ptr() + 4 * (off + col))


def _ray_distortion_range(rd):
    """(s_near, s_inv) of render_rays(ray_distortion=...) as two host floats; a value the kernels would refuse is refused here."""
    s_near, s_inv = float(rd[0]), float(rd[1])
    if not (np.isfinite(s_near) and np.isfinite(s_inv) and s_inv > 0.0):
        raise ValueError("nnr: ray_distortion=(s_near, s_inv) needs finite values and s_inv > 0, got %r" % ((s_near, s_inv),))
    return s_near, s_inv


GRAD_TAIL = 2048      # spare floats behind the flat weight-gradient buffer (see _RenderRays.backward)
_flat_grads = {}      # storage data_ptr -> (weak reference to the flat buffer, floats used by the gradient views): buffers _RenderRays.backward made


def register_flat_grads(flat: torch.Tensor, used: int):
    import weakref
    for k in [k for k, (r, _) in _flat_grads.items() if r() is None]:
        del _flat_grads[k]
    _flat_grads[flat.untyped_storage().data_ptr()] = (weakref.ref(flat), used)


def flat_grads_of(storage_ptr: int):
    """(flat buffer, used floats) if `storage_ptr` is the storage of a LIVE buffer made by _RenderRays.backward under data parallelism, else None."""
    hit = _flat_grads.get(storage_ptr)
    if hit is None or hit[0]() is None:
        return None
    return hit[0](), hit[1]


# ----------------------------------------------------------------------------------------------------------------------
# the frozen-field operator (include/nnr_frozen.h): the rays are differentiated, the field is a constant
# ----------------------------------------------------------------------------------------------------------------------
def _grid_args(grid, dev, what):
    """The grid of include/nnr_sparse.h as ctypes arguments: an object with lo, inv_step, dims and bits (model.geometry.OccupancyGrid)."""
    nx, ny, nz = (int(n) for n in grid.dims)
    bits = grid.bits
    if bits.dtype != torch.int32 or bits.device != dev or not bits.is_contiguous() or bits.numel() != nz * ny * ((nx + 31) // 32):
        raise ValueError("%s: grid.bits must be a contiguous int32 tensor of %d words on the rays' device; got %r %r on %s"
                         % (what, nz * ny * ((nx + 31) // 32), tuple(bits.shape), bits.dtype, bits.device))
    lo3 = (C.c_float * 3)(*[float(v) for v in grid.lo])
    is3 = (C.c_float * 3)(*[float(v) for v in grid.inv_step])
    d3 = (C.c_int32 * 3)(nx, ny, nz)
    return lo3, is3, d3, bits


def _frozen_sparse_fwd(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jit, grid, packed, ws, debug=False):
    """nnr_frozen_sparse_fwd on prepared tensors -> rgb, dist, alpha, z (and count, live, n_live under debug)."""
    dev = pts_o.device
    R, N = cfg.n_rays, cfg.n_samples
    f32 = dict(dtype=torch.float32, device=dev)
    lo3, is3, d3, bits = _grid_args(grid, dev, "render_frozen_sparse")
    rgb, dist = torch.empty(R, 3, **f32), torch.empty(R, **f32)
    alpha, zv = torch.empty(R, N, **f32), torch.empty(R, N, **f32)
    count = live = n_live = None
    if debug:
        count = torch.empty(R, dtype=torch.int32, device=dev)
        live = torch.full((R * N,), -1, dtype=torch.int32, device=dev)
        n_live = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(L.load().nnr_frozen_sparse_fwd(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(view_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3, is3,
                                           d3, L.ptr(bits), L.ptr(packed), L.ptr(rgb), L.ptr(dist), L.ptr(alpha), L.ptr(zv), L.ptr(count),
                                           L.ptr(live), L.ptr(n_live), L.ptr(ws), L.stream()), "nnr_frozen_sparse_fwd")
    return (rgb, dist, alpha, zv) + ((count, live, n_live) if debug else ())


frozen_sparse_tally = None      # tools: while this is a list, every sparse frozen forward of the operator appends (n_live (1) int32 tensor, R N)


def _frozen_bwd(cfg, kind, packed, d_rgb, d_dist, ws):
    """nnr_frozen_bwd or nnr_frozen_sparse_bwd, by the kind of workspace ("frozen" / "frozen_sparse") the forward filled -> d_pts_o, d_pts_d,
    d_view, (R,3) each.  An upstream gradient that is None counts as zero."""
    R = cfg.n_rays
    f32 = dict(dtype=torch.float32, device=ws.device)
    d_rgb = (d_rgb if d_rgb is not None else torch.zeros(R, 3, **f32)).contiguous().float()
    d_dist = (d_dist if d_dist is not None else torch.zeros(R, **f32)).contiguous().float()
    d_o, d_d, d_v = (torch.empty(R, 3, **f32) for _ in range(3))
    name = "nnr_%s_bwd" % kind
    L.check(getattr(L.load(), name)(C.byref(cfg), L.ptr(packed), L.ptr(d_rgb), L.ptr(d_dist), L.ptr(d_o), L.ptr(d_d), L.ptr(d_v), L.ptr(ws),
                                    L.stream()), name)
    return d_o, d_d, d_v


class _RenderRaysFrozen(torch.autograd.Function):
    """render_rays(frozen=True) where the frozen kernels apply: nnr_frozen_fwd / nnr_frozen_bwd on the frozen workspace, or -- with a grid in
    opts["occupancy"] -- nnr_frozen_sparse_fwd / nnr_frozen_sparse_bwd on the sparse one (include/nnr_frozen_sparse.h).  The parameters are
    not inputs of the node (they reach it through opts, for the pack cache): autograd has no edge to them, their .grad stay None.  The grid is
    the caller's object, valid because the caller says the field is frozen: it is never rebuilt or invalidated here."""

    @staticmethod
    def forward(ctx, pts_o, pts_d, view_d, z_lo, z_hi, jitter, opts):
        _require_gpu(pts_o)
        dev = pts_o.device
        R, N = pts_o.shape[0], z_lo.shape[0]
        cfg = L.make_cfg(R, N, opts["hidden"], dist_alpha=opts["dist_alpha"], white_bg=opts["white_bg"], relu_sigma=opts["relu_sigma"], train=True)
        (pts_o, pts_d, view_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d, view_d), z_lo, z_hi, jitter)
        packed = _packed_for(cfg, *opts["params"])
        grid = opts.get("occupancy")
        kind = "frozen" if grid is None else "frozen_sparse"
        ws = _take_workspace(cfg, dev, kind)
        if grid is None:
            f32 = dict(dtype=torch.float32, device=dev)
            rgb, dist = torch.empty(R, 3, **f32), torch.empty(R, **f32)
            alpha, zv = torch.empty(R, N, **f32), torch.empty(R, N, **f32)
            L.check(L.load().nnr_frozen_fwd(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(view_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit),
                                            L.ptr(packed), L.ptr(rgb), L.ptr(dist), L.ptr(alpha), L.ptr(zv), L.ptr(ws), L.stream()), "nnr_frozen_fwd")
        else:
            tally = frozen_sparse_tally
            res = _frozen_sparse_fwd(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jit, grid, packed, ws, debug=tally is not None)
            rgb, dist, alpha, zv = res[:4]
            if tally is not None:
                tally.append((res[6], R * N))      # (no synchronisation here: the reader sums the tensors afterwards)
        ctx.cfg, ctx.ws, ctx.kind, ctx.packed, ctx.dev = cfg, ws, kind, packed, dev
        ctx.mark_non_differentiable(alpha, zv)
        ctx.set_materialize_grads(False)
        return rgb, dist, alpha, zv

    @staticmethod
    def backward(ctx, d_rgb, d_dist, _da, _dz):
        cfg, ws = ctx.cfg, ctx.ws
        if ws is None:
            raise RuntimeError("nnr: backward called twice on the same render (workspace already released)")
        d_o, d_d, d_v = _frozen_bwd(cfg, ctx.kind, ctx.packed, d_rgb, d_dist, ws)
        ctx.ws = None
        _give_workspace(cfg, ctx.dev, ws, ctx.kind)      # to the pool of its own kind
        need = ctx.needs_input_grad
        return (d_o if need[0] else None, d_d if need[1] else None, d_v if need[2] else None, None, None, None, None)


def render_frozen_sparse(pts_o, pts_d, view_d, z_lo, z_hi, jitter, grid, weights, biases, *, hidden: int, dist_alpha: bool, white_bg: bool,
                         relu_sigma: bool, d_rgb=None, d_dist=None, debug: bool = False):
    """The sparse frozen-field render on plain tensors, no autograd (tests and tools; refinement goes through render_rays(frozen=True,
    occupancy=grid)): forward, and -- with d_rgb (R,3) and d_dist (R) -- backward.  Returns a dict: rgb, dist, alpha, z; d_pts_o, d_pts_d,
    d_view where the backward ran; count (R) int32, live (R N) int32 (-1 behind the list) and n_live (1) int32 under debug."""
    _require_gpu(pts_o)
    dev = pts_o.device
    R, N = pts_o.shape[0], z_lo.shape[0]
    cfg = split2_cfg(R, N, hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma, train=True)
    if white_bg:
        cfg.flags |= L.NNR_F_WHITE_BG
    (pts_o, pts_d, view_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d, view_d), z_lo, z_hi, jitter)
    packed = _packed_for(cfg, list(weights), list(biases))
    ws = _take_workspace(cfg, dev, "frozen_sparse")
    res = _frozen_sparse_fwd(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jit, grid, packed, ws, debug=debug)
    out = dict(zip(("rgb", "dist", "alpha", "z", "count", "live", "n_live"), res))
    if d_rgb is not None:
        out["d_pts_o"], out["d_pts_d"], out["d_view"] = _frozen_bwd(cfg, "frozen_sparse", packed, d_rgb, d_dist, ws)
    _give_workspace(cfg, dev, ws, "frozen_sparse")
    return out


_frozen_state = threading.local()      # .on: inside nnr.frozen_field() on this thread; .grid: its occupancy grid, if it was given one
_frozen_said = set()                   # the reasons already logged: one line each per process
_log = logging.getLogger("nnr")


@contextlib.contextmanager
def frozen_field(occupancy=None):
    """Inside the block, on this thread, every render_rays call with frozen=None behaves as frozen=True: the field's weights and biases are
    constants, the rays are differentiated (test-time pose refinement: model.Trainer_pose).  Nests; restores the previous state on exit.
    occupancy (default None): an occupancy grid of the field (model.geometry.OccupancyGrid, as render_sparse takes it); those calls then
    behave as render_rays(frozen=True, occupancy=grid).  The grid is the caller's: valid because the caller says the field is frozen."""
    prev = getattr(_frozen_state, "on", False), getattr(_frozen_state, "grid", None)
    _frozen_state.on, _frozen_state.grid = True, occupancy
    try:
        yield
    finally:
        _frozen_state.on, _frozen_state.grid = prev


def frozen_occupancy():
    """The occupancy grid of the enclosing nnr.frozen_field(occupancy=grid) on this thread, or None (outside such a block, or inside one
    that was given no grid): what a render_rays call with frozen=None would use.  For callers that run other kernels on the same frozen
    field, such as the renderer's sparse proposal (model/rendering.py)."""
    return getattr(_frozen_state, "grid", None) if getattr(_frozen_state, "on", False) else None


def _frozen_fallback_reason(pts_o, pts_d, view_d, bf16):
    """Why the frozen kernels do not apply to this call (None: they do).  They exist for the two-term fp16 products alone, and only a call
    that differentiates a ray input has a use for them."""
    if bf16:
        return "bf16=True has no frozen kernels"
    if L.fp32_products() != "split2":
        return "NNR_FP32_PRODUCTS=%s has no frozen kernels (only split2 has)" % L.fp32_products()
    if not torch.is_grad_enabled():
        return "gradients are disabled"
    if not any(t.requires_grad for t in (pts_o, pts_d, view_d)):
        return "no ray input requires a gradient"
    return None


def render_rays(pts_o: torch.Tensor, pts_d: torch.Tensor, view_d: torch.Tensor, z_lo: torch.Tensor, z_hi: torch.Tensor,
                jitter: Optional[torch.Tensor], weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], *,
                hidden: int, dist_alpha: bool, white_bg: bool, relu_sigma: bool, bf16: bool = False, samples: bool = True,
                ray_distortion=None, frozen: Optional[bool] = None, occupancy=None):
    """(R,3) sampling origin / direction / view direction, (N) z interval tables, optional (R,N) jitter, the 12
    nn.Linear weights and biases in state_dict order  ->  rgb (R,3), dist (R), alpha (R,N), z (R,N).
    Differentiable w.r.t. pts_o, pts_d, view_d, weights, biases.  bf16: bf16-MFMA products (fp32 accumulation) in the MLP
    forward and input-gradient kernels (NNR_F_BF16); weight gradients stay fp32.  samples=False (only honoured under torch.no_grad):
    alpha and z come back as None and the renderer composites inside the MLP kernel (16 bytes written per ray).
    ray_distortion=(s_near, s_inv) (default None: nothing changes): where gradients are needed, a fifth, differentiable output dloss (R,), the
    ray distortion of every ray's compositing weights at the normalised depths (z - s_near) * s_inv (include/nnr_regularise.h); its gradient
    reaches everything the other outputs' do.  Without gradients (torch.no_grad, or no input that requires one) the fifth output is None.
    frozen=True (default None: False, or True inside nnr.frozen_field()): the field is FROZEN -- weights and biases are constants, their
    gradients are None; outputs and the gradients of pts_o, pts_d, view_d are unchanged bit for bit.  The operator then runs the frozen
    kernels on the frozen workspace (include/nnr_frozen.h: no activation stash, no weight gradient, a workspace some 24 times smaller at
    hidden 256).  Where those do not apply (bf16=True, NNR_FP32_PRODUCTS other than split2, gradients disabled, no ray input that requires a
    gradient) today's kernels run with the weights detached, and one logged line (logger "nnr") says why.  Never inferred from requires_grad.
    frozen=True with ray_distortion raises ValueError: the regulariser is a training term.
    occupancy=grid (default None, or the grid of the enclosing nnr.frozen_field(occupancy=grid) where frozen is None; only with a frozen
    call, ValueError otherwise): an occupancy grid of the field (model.geometry.OccupancyGrid).  The frozen render then skips the samples in
    cells the grid calls empty, forward and backward (include/nnr_frozen_sparse.h): the render of a field whose culled
    samples hold no matter.  The grid is the caller's object and is never rebuilt or invalidated here.  Where the frozen kernels do not
    apply the grid is ignored, the dense path runs, and one logged line per reason says so."""
    if frozen is None:
        frozen = getattr(_frozen_state, "on", False)
        if frozen and occupancy is None:
            occupancy = getattr(_frozen_state, "grid", None)
    if occupancy is not None and not frozen:
        raise ValueError("nnr: render_rays(occupancy=grid) needs frozen=True (or nnr.frozen_field): the grid is only valid for a field that "
                         "does not move")
    if frozen and ray_distortion is not None:
        raise ValueError("nnr: render_rays(frozen=True) takes no ray_distortion: the regulariser is a term of the field's training")
    opts = dict(hidden=hidden, dist_alpha=dist_alpha, white_bg=white_bg, relu_sigma=relu_sigma, bf16=bool(bf16), samples=bool(samples),
                params=(list(weights), list(biases)))    # the caller's own tensor objects: identity keys the pack cache
    if ray_distortion is not None:
        opts["ray_distortion"] = _ray_distortion_range(ray_distortion)
    if frozen:
        why = _frozen_fallback_reason(pts_o, pts_d, view_d, bool(bf16))
        if why is None:
            opts["occupancy"] = occupancy
            return _RenderRaysFrozen.apply(pts_o, pts_d, view_d, z_lo, z_hi, jitter, opts)
        said = why if occupancy is None else why + " (the occupancy grid is ignored: every sample is rendered)"
        if said not in _frozen_said:
            _frozen_said.add(said)
            _log.info("nnr: render_rays(frozen=True) runs the training kernels with detached weights: %s", said)
        weights, biases = [w.detach() for w in weights], [b.detach() for b in biases]      # (opts["params"] keeps the caller's objects: the pack cache's key)
    if not torch.is_grad_enabled():
        # forward-only (eval / visualisation inside torch.no_grad): no stash, small workspace
        return _RenderRays.apply(pts_o.detach(), pts_d.detach(), view_d.detach(), z_lo, z_hi, jitter, opts,
                                 *[w.detach() for w in weights], *[b.detach() for b in biases])
    return _RenderRays.apply(pts_o, pts_d, view_d, z_lo, z_hi, jitter, opts, *weights, *biases)


def _ray_distortion_inputs(raw, z):
    _require_gpu(raw)
    _require_gpu(z)
    if raw.dim() != 2 or z.shape != raw.shape or raw.dtype != torch.float32 or z.dtype != torch.float32:
        raise ValueError("nnr: ray_distortion takes fp32 raw and z of one shape (R, N), got %r %s and %r %s"
                         % (tuple(raw.shape), raw.dtype, tuple(z.shape), z.dtype))
    if not z.is_contiguous():
        raise ValueError("nnr: ray_distortion: z must be contiguous")
    return _sample_stride(raw)


def _sample_stride(t: torch.Tensor) -> int:
    """Floats between consecutive samples of an (R, N) tensor whose element (r, j) sits (r N + j) strides behind the first."""
    R, N = t.shape
    s = t.stride(1) if N > 1 else (t.stride(0) if R > 1 else 1)
    if s < 1 or (R > 1 and t.stride(0) != s * N):
        raise ValueError("nnr: ray_distortion: an (R, N) tensor with ONE stride between consecutive samples is needed (a contiguous tensor, "
                         "or a column of an (R N, k) one viewed as (R, N)); got strides %r" % (tuple(t.stride()),))
    return s


def ray_distortion(raw: torch.Tensor, z: torch.Tensor, s_near: float, s_inv: float, dist_alpha: bool, relu_sigma: bool) -> torch.Tensor:
    """The ray distortion of (R, N) fp32 densities-before-activation `raw` at depths `z` (non-decreasing along a ray): loss (R,), the kernel of
    include/nnr_regularise.h alone on plain tensors (tests and tools; training goes through render_rays(ray_distortion=...)).  `raw` may be
    a strided view with one stride between samples: t[:, c].view(R, N) of an (R N, k) tensor.  No autograd: see ray_distortion_grad."""
    stride = _ray_distortion_inputs(raw, z)
    R, N = raw.shape
    cfg = L.make_cfg(R, N, 0, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    loss = torch.empty(R, dtype=torch.float32, device=raw.device)
    s_near, s_inv = _ray_distortion_range((s_near, s_inv))
    L.check(L.load().nnr_ray_distortion_fwd(C.byref(cfg), C.c_void_p(raw.data_ptr()), stride, L.ptr(z), s_near, s_inv, L.ptr(loss), L.stream()),
            "nnr_ray_distortion_fwd")
    return loss


def ray_distortion_grad(raw: torch.Tensor, z: torch.Tensor, s_near: float, s_inv: float, dist_alpha: bool, relu_sigma: bool, g: torch.Tensor,
                        out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """g_r d(loss_r)/d(raw_rj) of ray_distortion, (R, N) fp32.  `out` (default: a new contiguous tensor): where to write, laid out like `raw`
    may be; accumulate=True adds to what `out` holds (the sum formed in double, rounded once) instead of overwriting."""
    stride = _ray_distortion_inputs(raw, z)
    R, N = raw.shape
    _require_gpu(g)
    if g.shape != (R,) or g.dtype != torch.float32:
        raise ValueError("nnr: ray_distortion_grad: g must be fp32 of shape (R,)")
    if out is None:
        if accumulate:
            raise ValueError("nnr: ray_distortion_grad: accumulate=True needs `out`")
        out = torch.empty(R, N, dtype=torch.float32, device=raw.device)
    if out.shape != raw.shape or out.dtype != torch.float32:
        raise ValueError("nnr: ray_distortion_grad: out must be fp32 of raw's shape")
    _require_gpu(out)
    out_stride = _sample_stride(out)
    cfg = L.make_cfg(R, N, 0, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    s_near, s_inv = _ray_distortion_range((s_near, s_inv))
    L.check(L.load().nnr_ray_distortion_bwd(C.byref(cfg), C.c_void_p(raw.data_ptr()), stride, L.ptr(z), s_near, s_inv, L.ptr(g.contiguous()),
                                            C.c_void_p(out.data_ptr()), out_stride, int(bool(accumulate)), L.stream()),
            "nnr_ray_distortion_bwd")
    return out


def mlp_points(pts: torch.Tensor, view: torch.Tensor, weights, biases, *, hidden: int, split2: bool = False):
    """Forward-only evaluation of the MLP on free-standing points: (S,3),(S,3) -> rgb (S,3), sigma_raw (S,).
    Each point is rendered as a one-sample ray (origin = point, direction = 0) through the same fused kernel.
    split2: the two-term fp16 products whatever lib.set_fp32_products selects (the phong renderer's mode)."""
    _require_gpu(pts)
    S, dev = pts.shape[0], pts.device
    cfg = split2_cfg(S, 1, hidden) if split2 else L.make_cfg(S, 1, hidden)
    lib = L.load()
    pts = pts.detach().contiguous().float()
    view = view.detach().contiguous().float()
    zeros3 = torch.zeros_like(pts)
    z0 = torch.zeros(1, dtype=torch.float32, device=dev)
    packed = _packed_for(cfg, list(weights), list(biases))
    ws = _take_workspace(cfg, dev)
    st = L.stream()
    L.check(lib.nnr_mlp_fwd(C.byref(cfg), L.ptr(pts), L.ptr(zeros3), L.ptr(view), L.ptr(z0), L.ptr(z0), None,
                            L.ptr(packed), L.ptr(ws), st), "nnr_mlp_fwd")
    out = workspace_plane(cfg, ws, 0).clone()
    _give_workspace(cfg, dev, ws)
    return out[:, :3], out[:, 3]


# ----------------------------------------------------------------------------------------------------------------------
# the phong geometry renderer (model/rendering.py: Renderer.phong_renderer): the depth search and the surface normals
# ----------------------------------------------------------------------------------------------------------------------
def split2_cfg(n_rays: int, n_samples: int, hidden: int, *, dist_alpha=False, relu_sigma=False, train=False) -> L.Cfg:
    """A cfg in the two-term fp16 mode (NNR_F_SPLIT3 | NNR_F_SPLIT2) regardless of lib.set_fp32_products: the phong renderer always
    evaluates in this mode (its march kernel exists only in it), so its output does not depend on the training step's product setting."""
    flags = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2 | (L.NNR_F_DIST_ALPHA if dist_alpha else 0) | (L.NNR_F_RELU_SIGMA if relu_sigma else 0) | \
        (L.NNR_F_TRAIN if train else 0)
    return L.Cfg(int(n_rays), int(n_samples), int(hidden), flags)


def ray_march(ray_o: torch.Tensor, ray_d: torch.Tensor, t_table: torch.Tensor, weights, biases, *, hidden: int, radius: float,
              n_secant: int = 8, relu_sigma: bool = False, dist_alpha: bool = False) -> torch.Tensor:
    """The reference's ray_marching + secant (model/rendering.py:277-418) in 2 + n_secant launches of nnr_ray_march: (R,3) origins,
    (R,3) unit directions, the (n_steps) torch.linspace(0, 1, n_steps) table on the device -> d (R): the surface depth on a hit, +inf on a
    miss, 0 where the first proposal is occupied.  No host synchronisation."""
    _require_gpu(ray_o)
    R, dev = ray_o.shape[0], ray_o.device
    cfg = split2_cfg(R, t_table.shape[0], hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    lib = L.load()
    ray_o = ray_o.detach().contiguous().float()
    ray_d = ray_d.detach().contiguous().float()
    t_table = t_table.detach().contiguous().float()
    packed = _packed_for(cfg, list(weights), list(biases))
    state = torch.empty(R, 4, dtype=torch.float32, device=dev)
    d = torch.empty(R, dtype=torch.float32, device=dev)
    L.check(lib.nnr_ray_march(C.byref(cfg), L.ptr(ray_o), L.ptr(ray_d), float(radius), L.ptr(t_table), int(n_secant), L.ptr(packed),
                              L.ptr(state), L.ptr(d), L.stream()), "nnr_ray_march")
    return d


def density_grid(origin, step, dims, weights, biases, *, hidden: int) -> torch.Tensor:
    """The raw density (sigma_raw, before softplus / relu) on a regular grid in one launch of nnr_density_grid (include/nnr.h): origin, step
    (three floats each), dims = (nx, ny, nz) -> (nz, ny, nx) fp32 on the weights' device.  Voxel (ix, iy, iz) is the point
    origin + step * (ix, iy, iz), product and sum rounded to fp32 separately; the points are made in the kernel, nothing per point is read.
    The value is mlp_points(p, ., split2=True)[1] at that point, bit for bit.  Always in the two-term fp16 products (split2_cfg); the pack is
    cached per parameter identity, as for propose.  Not differentiable.  No host synchronisation."""
    weights, biases = list(weights), list(biases)
    _require_gpu(weights[0])
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 1 or nx * ny * nz > 2 ** 31 - 1:
        raise ValueError("density_grid: dims %r: every dim >= 1 and at most 2^31 - 1 voxels in one call (model.geometry.density_volume "
                         "walks a larger volume in slabs)" % ((nx, ny, nz),))
    cfg = split2_cfg(nx * ny * nz, 1, hidden)
    packed = _packed_for(cfg, weights, biases)
    out = torch.empty(nz, ny, nx, dtype=torch.float32, device=weights[0].device)
    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    s3 = (C.c_float * 3)(*[float(v) for v in step])
    d3 = (C.c_int32 * 3)(nx, ny, nz)
    L.check(L.load().nnr_density_grid(C.byref(cfg), o3, s3, d3, L.ptr(packed), L.ptr(out), L.stream()), "nnr_density_grid")
    return out


def density_bricks(origin, step, bricks: torch.Tensor, weights, biases, *, hidden: int) -> torch.Tensor:
    """The raw density in a list of 8 x 8 x 8 bricks of the grid (origin, step) in one launch of nnr_density_bricks (include/nnr_geometry.h):
    bricks (B,3) int32 on the weights' device, (bx, by, bz) per brick, non-negative -> (B, 8, 8, 8) fp32, [b][lz][ly][lx]: the grid point
    (8 bx + lx, 8 by + ly, 8 bz + lz).  Every voxel is density_grid's value at the same grid point, bit for bit.  Bricks may repeat and come in
    any order; the grid has no dims here, a brick that reaches past its last point is evaluated all the same.  Always in the two-term fp16
    products (split2_cfg), with the cached pack, as density_grid.  Not differentiable.  No host synchronisation."""
    weights, biases = list(weights), list(biases)
    _require_gpu(weights[0])
    if bricks.dtype != torch.int32 or bricks.dim() != 2 or bricks.shape[1] != 3 or bricks.device != weights[0].device:
        raise ValueError("density_bricks: bricks must be a (B,3) int32 tensor on the weights' device; got %r %r on %s"
                         % (tuple(bricks.shape), bricks.dtype, bricks.device))
    B = bricks.shape[0]
    if B < 1 or 512 * B > 2 ** 31 - 1:
        raise ValueError("density_bricks: %d bricks: at least one and at most %d (2^31 - 1 voxels) in one call" % (B, (2 ** 31 - 1) // 512))
    cfg = split2_cfg(512 * B, 1, hidden)
    packed = _packed_for(cfg, weights, biases)
    bricks = bricks.contiguous()
    out = torch.empty(B, 8, 8, 8, dtype=torch.float32, device=weights[0].device)
    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    s3 = (C.c_float * 3)(*[float(v) for v in step])
    L.check(L.load().nnr_density_bricks(C.byref(cfg), o3, s3, L.ptr(bricks), B, L.ptr(packed), L.ptr(out), L.stream()), "nnr_density_bricks")
    return out


def _quantile_level(level, what):
    """quantile_level of the depth renders: None, or a float the fp32 of which lies in (0, 1)"""
    if level is None:
        return None
    level = float(level)
    if not 0.0 < C.c_float(level).value < 1.0:      # (a NaN fails)
        raise ValueError("%s: quantile_level must be in (0, 1); got %r" % (what, level))
    return level


def render_depth(pts_o: torch.Tensor, pts_d: torch.Tensor, z_lo: torch.Tensor, z_hi: torch.Tensor, jitter: Optional[torch.Tensor], weights, biases, *,
                 hidden: int, dist_alpha: bool, relu_sigma: bool, debug: bool = False, quantile_level: Optional[float] = None):
    """The rendered depth of rays from the density alone in one launch of nnr_render_depth (include/nnr_fusion.h): the inputs of a render_rays
    call without the view direction -> (R,2) fp32, (depth, acc) per ray: depth = sum w_j z_j and acc = sum w_j over the compositor's weights.
    No colour branch, nothing per sample written to HBM.  Always in the two-term fp16 products (split2_cfg), with the cached pack, as propose.
    (NaN, NaN) for a ray with a NaN sample.  debug: (out, raw (R,C), z (R,C)), the samples' raw densities and depths.  1 <= C <= 256.
    quantile_level (None: the call above): a float in (0, 1) -> (R,3), (depth, acc, q) in one launch of nnr_render_depth_median
    (include/nnr_depth_median.h): q the depth at which the ray's transmittance falls below the level (0.5: the median depth), +inf where it
    never does; depth and acc are bit for bit the two columns above.
    Not differentiable.  No host synchronisation."""
    level = _quantile_level(quantile_level, "render_depth")
    _require_gpu(pts_o)
    R, Cn = pts_o.shape[0], z_lo.shape[0]
    dev = pts_o.device
    cfg = split2_cfg(R, Cn, hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    (pts_o, pts_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d), z_lo, z_hi, jitter)
    packed = _packed_for(cfg, list(weights), list(biases))
    f32 = dict(dtype=torch.float32, device=dev)
    out = torch.empty(R, 2 if level is None else 3, **f32)
    raw, zv = (torch.empty(R, Cn, **f32), torch.empty(R, Cn, **f32)) if debug else (None, None)
    if level is None:
        L.check(L.load().nnr_render_depth(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), L.ptr(packed), L.ptr(out),
                                          L.ptr(raw), L.ptr(zv), L.stream()), "nnr_render_depth")
    else:
        L.check(L.load().nnr_render_depth_median(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), level,
                                                 L.ptr(packed), L.ptr(out), L.ptr(raw), L.ptr(zv), L.stream()), "nnr_render_depth_median")
    return (out, raw, zv) if debug else out


def render_sparse(pts_o: torch.Tensor, pts_d: torch.Tensor, view_d: torch.Tensor, z_lo: torch.Tensor, z_hi: torch.Tensor,
                  jitter: Optional[torch.Tensor], grid, weights, biases, *, hidden: int, dist_alpha: bool, white_bg: bool, relu_sigma: bool,
                  t_min: float = 0.0, debug: bool = False):
    """A forward-only render that evaluates the MLP only on the samples an occupancy grid does not call empty, in one launch of
    nnr_render_sparse (include/nnr_sparse.h): the inputs of a render_rays call plus `grid` -- an object with lo, inv_step (three floats each),
    dims = (n_x, n_y, n_z) cells and bits, the (n_z, n_y, ceil(n_x / 32)) int32 words on the rays' device (model.geometry.OccupancyGrid) ->
    rgb (R,3), dist (R) = sum w z, acc (R) = sum w.  A sample outside the grid, or in a cell whose bit is set, is evaluated and composited with
    the alpha it has in the dense render; a sample in a cell whose bit is clear is skipped.  Always in the two-term fp16 products
    (split2_cfg), with the cached pack, as propose.  debug: (rgb, dist, acc, count (R) int32, cell (R,C) int32, out4 (R,C,4) with NaN rows for
    the culled samples).  Any R, 1 <= C <= 256.  Not differentiable.  No host synchronisation.
    t_min (0 <= t_min < 1; default 0: off, nnr_render_sparse exactly as without it): early ray termination, one launch of
    nnr_render_sparse_stop (include/nnr_sparse_stop.h) -- a workgroup of four rays stops walking their live lists, 32 samples a pass, once
    each ray's list is exhausted or its transmittance is below t_min; a ray's outputs come from the samples evaluated until then and differ
    from the unstopped ones by at most about t_min (times the largest z for dist).  debug then also returns, as a seventh element, passes (R)
    int32: the passes the ray's workgroup ran; out4 keeps NaN rows for the live samples that were not evaluated."""
    t_min = float(t_min)
    if not 0.0 <= t_min < 1.0:      # (a NaN fails)
        raise ValueError("render_sparse: t_min must be in [0, 1); got %r" % (t_min,))
    _require_gpu(pts_o)
    R, Cn = pts_o.shape[0], z_lo.shape[0]
    dev = pts_o.device
    cfg = split2_cfg(R, Cn, hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    if white_bg:
        cfg.flags |= L.NNR_F_WHITE_BG
    (pts_o, pts_d, view_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d, view_d), z_lo, z_hi, jitter)
    lo3, is3, d3, bits = _grid_args(grid, dev, "render_sparse")
    packed = _packed_for(cfg, list(weights), list(biases))
    out = torch.empty(R, 5, dtype=torch.float32, device=dev)
    count = cell = out4 = None
    if debug:
        count = torch.empty(R, dtype=torch.int32, device=dev)
        cell = torch.empty(R, Cn, dtype=torch.int32, device=dev)
        out4 = torch.full((R, Cn, 4), float("nan"), dtype=torch.float32, device=dev)
    if t_min > 0.0:
        passes = torch.empty(R, dtype=torch.int32, device=dev) if debug else None
        L.check(L.load().nnr_render_sparse_stop(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(view_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3, is3,
                                                d3, L.ptr(bits), L.ptr(packed), t_min, L.ptr(out), L.ptr(count), L.ptr(cell), L.ptr(out4),
                                                L.ptr(passes), L.stream()), "nnr_render_sparse_stop")
        res = (out[:, :3], out[:, 3], out[:, 4])
        return res + (count, cell, out4, passes) if debug else res
    L.check(L.load().nnr_render_sparse(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(view_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3, is3, d3,
                                       L.ptr(bits), L.ptr(packed), L.ptr(out), L.ptr(count), L.ptr(cell), L.ptr(out4), L.stream()),
            "nnr_render_sparse")
    res = (out[:, :3], out[:, 3], out[:, 4])
    return res + (count, cell, out4) if debug else res


class ParamsStamp:
    """What a packed-weights cache entry is valid for, for whoever derives something else from the parameters (the renderer's occupancy
    grid): the very same tensor objects at the same in-place versions, with no optimizer step since."""

    def __init__(self, weights, biases):
        self._entry = _PackCache(None, [*weights, *biases], None)

    def matches(self, weights, biases):
        return self._entry.matches(None, [*weights, *biases])


def tsdf_integrate(origin, step, bricks: torch.Tensor, cams: torch.Tensor, depth: torch.Tensor, trunc: float, sum: torch.Tensor,
                   weight: torch.Tensor, z_min: float = 0.):
    """Integrate depth maps into the truncated signed distance accumulators of a list of 8 x 8 x 8 bricks of the grid (origin, step), IN PLACE,
    in one launch of nnr_tsdf_integrate (include/nnr_fusion.h): bricks (B,3) int32 as density_bricks takes them, cams (n,12) fp32 (rows 0..2 of
    K . world_mat . scale_mat: model.geometry.projection_rows), depth (n,H,W) fp32 z-depth (NaN, 0 and negative: unobserved; +inf: free space),
    sum and weight (B,8,8,8) fp32, all on one GPU.  Per voxel and camera, in index order: sum += max((q_z - d) / trunc, -1), weight += 1 where
    the voxel projects into the image in front of z_min and lies no further than trunc behind the depth d of its pixel.  Cameras may come in
    chunks over several calls: the result is the one-call result bit for bit.  Returns (sum, weight).  No host synchronisation."""
    _require_gpu(sum)
    dev = sum.device
    if bricks.dtype != torch.int32 or bricks.dim() != 2 or bricks.shape[1] != 3 or bricks.device != dev:
        raise ValueError("tsdf_integrate: bricks must be a (B,3) int32 tensor on the accumulators' device; got %r %r on %s"
                         % (tuple(bricks.shape), bricks.dtype, bricks.device))
    B = bricks.shape[0]
    if B < 1 or 512 * B > 2 ** 31 - 1:
        raise ValueError("tsdf_integrate: %d bricks: at least one and at most %d (2^31 - 1 voxels) in one call" % (B, (2 ** 31 - 1) // 512))
    if cams.dim() != 2 or cams.shape[1] != 12 or depth.dim() != 3 or depth.shape[0] != cams.shape[0] or cams.shape[0] < 1:
        raise ValueError("tsdf_integrate: cams (n,12) and depth (n,H,W), n >= 1; got %r and %r" % (tuple(cams.shape), tuple(depth.shape)))
    for name, t in (("cams", cams), ("depth", depth), ("sum", sum), ("weight", weight)):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError("tsdf_integrate: %s must be a contiguous fp32 tensor on the accumulators' device" % name)
    if tuple(sum.shape) != (B, 8, 8, 8) or tuple(weight.shape) != (B, 8, 8, 8):
        raise ValueError("tsdf_integrate: sum and weight must be (%d, 8, 8, 8); got %r and %r" % (B, tuple(sum.shape), tuple(weight.shape)))
    n, H, W = depth.shape
    bricks = bricks.contiguous()
    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    s3 = (C.c_float * 3)(*[float(v) for v in step])
    L.check(L.load().nnr_tsdf_integrate(o3, s3, L.ptr(bricks), B, L.ptr(cams), n, L.ptr(depth), H, W, float(trunc), float(z_min), L.ptr(sum),
                                        L.ptr(weight), L.stream()), "nnr_tsdf_integrate")
    return sum, weight


_P_DOUT4, _P_DPTS = 2, 3     # workspace planes (nnr_layout.h): the per-sample output gradient, the gradient of the sample's point


def density_grad(points: torch.Tensor, weights, biases, hidden: int) -> torch.Tensor:
    """d(raw density)/d(point) for (S,3) points -> (S,3), first order, with the training kernels and no new MLP code: one training
    forward with one-sample rays (origin = point, direction = 0, as mlp_points), the output-gradient plane seeded with (0, 0, 0, 1) --
    d rgb_pre = 0, d sigma_raw = 1, the one plane of the composite backward the input-gradient kernel reads -- then nnr_mlp_dgrad; the
    answer is its d(point) plane.  Two-term fp16 products (split2_cfg)."""
    _require_gpu(points)
    S, dev = points.shape[0], points.device
    cfg = split2_cfg(S, 1, hidden, train=True)
    lib = L.load()
    pts = points.detach().contiguous().float()
    zeros3 = torch.zeros_like(pts)
    z0 = torch.zeros(1, dtype=torch.float32, device=dev)
    packed = _packed_for(cfg, list(weights), list(biases))
    ws = _take_workspace(cfg, dev)
    st = L.stream()
    L.check(lib.nnr_mlp_fwd(C.byref(cfg), L.ptr(pts), L.ptr(zeros3), L.ptr(zeros3), L.ptr(z0), L.ptr(z0), None,
                            L.ptr(packed), L.ptr(ws), st), "nnr_mlp_fwd")
    seed = workspace_plane(cfg, ws, _P_DOUT4)
    seed[:, :3] = 0.
    seed[:, 3] = 1.
    L.check(lib.nnr_mlp_dgrad(C.byref(cfg), L.ptr(packed), L.ptr(ws), st), "nnr_mlp_dgrad")
    g = workspace_plane(cfg, ws, _P_DPTS)[:, :3].clone()
    _give_workspace(cfg, dev, ws)
    return g


# ----------------------------------------------------------------------------------------------------------------------
# hierarchical sampling (model/rendering.py: rendering.num_fine)
# ----------------------------------------------------------------------------------------------------------------------
def resample(alpha: torch.Tensor, z: torch.Tensor, xi: Optional[torch.Tensor], n_fine: int, return_fine: bool = False):
    """alpha, z (R,C) of a coarse render (render_rays' per-sample outputs), xi (R,n_fine) in [0,1) or None (= 0.5) -> z_all (R, C + n_fine):
    per ray the coarse depths and n_fine inverse-CDF samples of the compositor's weights, merged and sorted (nnr_resample, include/nnr.h).
    return_fine: also the (R,n_fine) fine samples on their own.  Not differentiable (the depths carry no gradient).  One launch, no host
    synchronisation."""
    _require_gpu(alpha)
    R, Cn = alpha.shape
    F = int(n_fine)
    dev = alpha.device
    alpha = alpha.detach().contiguous().float()
    z = z.detach().contiguous().float().view(R, Cn)
    xi = xi.detach().contiguous().float().view(R, F) if xi is not None else None
    z_all = torch.empty(R, Cn + max(F, 0), dtype=torch.float32, device=dev)
    fine = torch.empty(R, max(F, 0), dtype=torch.float32, device=dev) if return_fine else None
    L.check(L.load().nnr_resample(R, Cn, F, L.ptr(alpha), L.ptr(z), L.ptr(xi), L.ptr(z_all), L.ptr(fine), L.stream()), "nnr_resample")
    return (z_all, fine) if return_fine else z_all


def propose(pts_o: torch.Tensor, pts_d: torch.Tensor, z_lo: torch.Tensor, z_hi: torch.Tensor, jitter: Optional[torch.Tensor],
            xi: Optional[torch.Tensor], n_fine: int, weights, biases, *, hidden: int, dist_alpha: bool, relu_sigma: bool, debug: bool = False):
    """The proposal stage of hierarchical sampling in one launch (nnr_propose, include/nnr.h; rendering.proposal: 'density'): the inputs of the
    coarse render_rays call without the view direction, xi (R,n_fine) in [0,1) or None (= 0.5) -> z_all (R, C + n_fine), what
    resample(alpha, z, xi, n_fine) gives for the alpha, z of that coarse render -- from the density alone (no colour branch), with nothing per
    sample written to HBM.  Always in the two-term fp16 products (split2_cfg), whatever the training step uses, as the phong renderer; the pack
    is cached per parameter identity.  debug: (z_all, alpha_c (R,C), z_c (R,C), fine (R,n_fine)), the kernel's own intermediate rows.
    Not differentiable (the depths carry no gradient).  3 <= C <= 256, C + n_fine <= 1024.  No host synchronisation."""
    _require_gpu(pts_o)
    R, Cn = pts_o.shape[0], z_lo.shape[0]
    F = int(n_fine)
    dev = pts_o.device
    cfg = split2_cfg(R, Cn, hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    (pts_o, pts_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d), z_lo, z_hi, jitter)
    xi = xi.detach().contiguous().float().view(R, F) if xi is not None else None
    packed = _packed_for(cfg, list(weights), list(biases))
    f32 = dict(dtype=torch.float32, device=dev)
    z_all = torch.empty(R, Cn + max(F, 0), **f32)
    alpha_c, z_c, fine = ((torch.empty(R, Cn, **f32), torch.empty(R, Cn, **f32), torch.empty(R, max(F, 0), **f32)) if debug
                          else (None, None, None))
    L.check(L.load().nnr_propose(C.byref(cfg), F, L.ptr(pts_o), L.ptr(pts_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), L.ptr(xi), L.ptr(packed),
                                 L.ptr(z_all), L.ptr(alpha_c), L.ptr(z_c), L.ptr(fine), L.stream()), "nnr_propose")
    return (z_all, alpha_c, z_c, fine) if debug else z_all


propose_sparse_tally = None      # tools: while this is a list, every propose_sparse call appends (live coarse samples (1) tensor, R C)


def propose_sparse(pts_o: torch.Tensor, pts_d: torch.Tensor, z_lo: torch.Tensor, z_hi: torch.Tensor, jitter: Optional[torch.Tensor],
                   xi: Optional[torch.Tensor], n_fine: int, grid, weights, biases, *, hidden: int, dist_alpha: bool, relu_sigma: bool,
                   debug: bool = False):
    """propose that does not evaluate the coarse samples an occupancy grid calls empty, in one launch of nnr_propose_sparse
    (include/nnr_propose_sparse.h; rendering.occupancy.proposal): propose's inputs plus `grid`, as render_sparse takes it -> z_all
    (R, C + n_fine), bit for bit what resample(alpha', z, xi, n_fine) gives, alpha' being propose's alpha where the sample is live (outside
    the grid, or in a cell whose bit is set) and 0 where it is culled.  With every bit set that is propose's output bit for bit; a ray
    without a live sample gets the row resample makes from zeros.  A culled sample is not evaluated and so cannot make its ray NaN.  The
    cached pack, as propose.  debug: (z_all, alpha_c (R,C) = alpha', z_c (R,C), fine (R,n_fine), count (R) int32, cell (R,C) int32,
    passes (R) int32: the passes of 32 samples the ray's workgroup of four rays ran).  Not differentiable.  3 <= C <= 256,
    C + n_fine <= 1024.  No host synchronisation."""
    _require_gpu(pts_o)
    R, Cn = pts_o.shape[0], z_lo.shape[0]
    F = int(n_fine)
    dev = pts_o.device
    cfg = split2_cfg(R, Cn, hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    (pts_o, pts_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d), z_lo, z_hi, jitter)
    xi = xi.detach().contiguous().float().view(R, F) if xi is not None else None
    lo3, is3, d3, bits = _grid_args(grid, dev, "propose_sparse")
    packed = _packed_for(cfg, list(weights), list(biases))
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    z_all = torch.empty(R, Cn + max(F, 0), **f32)
    alpha_c = z_c = fine = count = cell = passes = None
    tally = propose_sparse_tally
    if debug:
        alpha_c, z_c, fine = torch.empty(R, Cn, **f32), torch.empty(R, Cn, **f32), torch.empty(R, max(F, 0), **f32)
        count, cell, passes = torch.empty(R, **i32), torch.empty(R, Cn, **i32), torch.empty(R, **i32)
    elif tally is not None:
        count = torch.empty(R, **i32)
    L.check(L.load().nnr_propose_sparse(C.byref(cfg), F, L.ptr(pts_o), L.ptr(pts_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), L.ptr(xi), lo3, is3, d3,
                                        L.ptr(bits), L.ptr(packed), L.ptr(z_all), L.ptr(alpha_c), L.ptr(z_c), L.ptr(fine), L.ptr(count),
                                        L.ptr(cell), L.ptr(passes), L.stream()), "nnr_propose_sparse")
    if tally is not None:
        tally.append((count.sum(), R * Cn))
    return (z_all, alpha_c, z_c, fine, count, cell, passes) if debug else z_all


depth_sparse_tally = None      # tools: while this is a list, every render_depth_sparse call appends (live samples (1), passes summed over rays (1), R C, R)


def render_depth_sparse(pts_o: torch.Tensor, pts_d: torch.Tensor, z_lo: torch.Tensor, z_hi: torch.Tensor, jitter: Optional[torch.Tensor], grid,
                        weights, biases, *, hidden: int, dist_alpha: bool, relu_sigma: bool, t_min: float = 0.0, debug: bool = False,
                        quantile_level: Optional[float] = None):
    """render_depth that does not evaluate the samples an occupancy grid calls empty and stops a workgroup of four rays once they are opaque,
    in one launch of nnr_render_depth_sparse (include/nnr_depth_sparse.h): render_depth's inputs plus `grid`, as render_sparse takes it ->
    (R,2) fp32, (depth, acc) per ray over the evaluated samples -- bit for bit the dist and acc render_sparse(..., t_min=t_min) gives the
    same rays, without its colour branch, view direction and rgb.  A ray without a live sample gets (0, 0); a culled or unevaluated sample
    cannot make its ray NaN.  t_min (0 <= t_min < 1; 0: the full lists run): as render_sparse's.  The cached pack, as propose.
    debug: (out, raw (R,C) pre-filled with NaN and written at the evaluated samples alone, count (R) int32, cell (R,C) int32, passes (R)
    int32).  Any R, 1 <= C <= 256.
    quantile_level (None: the call above): a float in (0, 1), t_min <= quantile_level -> (R,3), (depth, acc, q) in one launch of
    nnr_render_depth_median_sparse (include/nnr_depth_median.h): q the depth at which the transmittance over the evaluated samples falls
    below the level, +inf where it never does -- the same bits at every t_min up to the level; everything else is the call above's bit
    for bit at the same t_min.
    Not differentiable.  No host synchronisation."""
    t_min = float(t_min)
    if not 0.0 <= t_min < 1.0:      # (a NaN fails)
        raise ValueError("render_depth_sparse: t_min must be in [0, 1); got %r" % (t_min,))
    level = _quantile_level(quantile_level, "render_depth_sparse")
    if level is not None and C.c_float(t_min).value > C.c_float(level).value:
        raise ValueError("render_depth_sparse: t_min = %r above quantile_level = %r: a ray stopped there has not crossed the level" % (t_min, level))
    _require_gpu(pts_o)
    R, Cn = pts_o.shape[0], z_lo.shape[0]
    dev = pts_o.device
    cfg = split2_cfg(R, Cn, hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma)
    (pts_o, pts_d), z_lo, z_hi, jit = _ray_inputs((pts_o, pts_d), z_lo, z_hi, jitter)
    lo3, is3, d3, bits = _grid_args(grid, dev, "render_depth_sparse")
    packed = _packed_for(cfg, list(weights), list(biases))
    out = torch.empty(R, 2 if level is None else 3, dtype=torch.float32, device=dev)
    raw = count = cell = passes = None
    if debug:
        raw = torch.full((R, Cn), float("nan"), dtype=torch.float32, device=dev)
        count, passes = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
        cell = torch.empty(R, Cn, dtype=torch.int32, device=dev)
    tally = depth_sparse_tally
    if tally is not None and not debug:
        count, passes = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    if level is None:
        L.check(L.load().nnr_render_depth_sparse(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3, is3, d3,
                                                 L.ptr(bits), t_min, L.ptr(packed), L.ptr(out), L.ptr(raw), L.ptr(count), L.ptr(cell),
                                                 L.ptr(passes), L.stream()), "nnr_render_depth_sparse")
    else:
        L.check(L.load().nnr_render_depth_median_sparse(C.byref(cfg), L.ptr(pts_o), L.ptr(pts_d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3, is3,
                                                        d3, L.ptr(bits), t_min, level, L.ptr(packed), L.ptr(out), L.ptr(raw), L.ptr(count),
                                                        L.ptr(cell), L.ptr(passes), L.stream()), "nnr_render_depth_median_sparse")
    if tally is not None:
        tally.append((count.sum(), passes.sum(), R * Cn, R))
    return (out, raw, count, cell, passes) if debug else out
