"""Renderer -- host side of the volumetric-rendering hot path.

Same constructor, `forward` dispatch and output dictionary as the reference's model/rendering.py:11-34,159-166, but
the body of `nope_nerf` (reference :36-167) is: a few O(R) torch ops that turn (pixels, depth, K, W, S) into per-ray
sampling origins/directions inside the autograd graph (so gradients reach the learnable pose / focal / depth
distortion exactly as they do through the reference's matrix inverses), and ONE call into the fused HIP operator
`nnr.render_rays` for everything per-sample: stratified / NDC sampling, positional encoding, the 12-layer MLP,
alpha-compositing, and their backward.

`rendering.num_fine: F` (default 0 = off; the reference has no counterpart) turns the render into NeRF's hierarchical sampling with one
network: a coarse forward-only pass at the `num_points - outside_steps` samples above, `nnr.ops.resample` (nnr_resample.hip) for F more
depths per ray from the coarse weights' inverse CDF, and the render proper -- the training path -- at the sorted union of both sets.
`rendering.proposal: 'density'` (default 'render'; no reference counterpart either) replaces the coarse pass and the resampling launch by
one launch of the fused proposal kernel (`nnr.ops.propose`, nnr_propose_f16.hip): the density of the coarse samples alone.
`rendering.occupancy.proposal: true` (default false) makes that launch skip the coarse samples the render's occupancy grid calls empty
(`nnr.ops.propose_sparse`), wherever such a grid applies -- the sparse inference render's, or the one of `nnr.frozen_field(occupancy=grid)`.

`rendering.normal_loss: True` (reference :133-143; off by default, and no loss term of the reference consumes it) adds the
normal-consistency vector `out['normal']`: second-order autograd through the MLP trunk for the 2 M surface points, in stock torch
over the same nn.Linear parameters (OfficialStaticNerf.gradient) -- the fused kernels still render.

The phong geometry visualiser (`phong_renderer`, `ray_marching`, `secant`; reference :202-418) runs on the GPU: the occupancy march and
its secant steps in one HIP kernel (nnr_march_f16.hip via nnr.ops.ray_march), the normals through the training kernels
(nnr.ops.density_grad), always in the two-term fp16 products.  On CPU tensors they raise NotImplementedError.
"""
import logging

import torch
import torch.nn as nn

import nnr
from nnr import camera
from nnr import ops as _nnr_ops
from .common import get_ndc_rays_fxfy, pixel_to_world_matrix

epsilon = 1e-6   # the transmittance epsilon of the reference (rendering.py:9) -- applied inside the composite kernel


class RenderOutput(dict):
    """The renderer's output dictionary (reference rendering.py:159-166).  `depth_pred` / `depth_gt` -- the per-ray
    values compacted by the validity mask -- are materialised on first access: boolean-mask indexing costs a dozen small
    kernels and a device->host sync, and the trainer's fused loss works on the dense tensors + mask instead
    (keys `dist_dense`, `d_gt_dense`, `mask`)."""

    _LAZY = ('depth_pred', 'depth_gt', 'alpha', 'z_vals')

    def __missing__(self, key):
        if key not in self._LAZY:
            raise KeyError(key)
        if key in ('alpha', 'z_vals'):
            # forward-only renders composite inside the MLP kernel and write nothing per sample; whoever does want the per-sample
            # weights of an evaluation render gets them from a second, unfused pass
            self['alpha'], self['z_vals'] = dict.__getitem__(self, '_samples')()
            return dict.__getitem__(self, key)
        mask = dict.__getitem__(self, 'mask')
        if key == 'depth_pred':
            val = dict.__getitem__(self, 'dist_dense')[mask]
        else:
            val = dict.__getitem__(self, 'd_gt_dense')[mask]
            if dict.__getitem__(self, 'ndc'):
                val = 1 - 1 / val                                                   # rendering.py:157-158
        self[key] = val
        return val

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._LAZY

    def get(self, key, default=None):
        return self[key] if key in self else default


def _forward_only_samples(pts_o, pts_d, view, z_lo, z_hi, jitter, net, kw):
    """alpha / z_vals of an evaluation render, fetched late.  Under torch.no_grad() whatever the caller's mode is by then: read after the
    caller's no_grad block has ended, the operator would otherwise see grad-requiring weights and take the TRAINING path (full
    activation stash, a multi-GB workspace pinned by an autograd node) for two tensors nobody differentiates."""
    with torch.no_grad():
        return nnr.render_rays(pts_o, pts_d, view, z_lo, z_hi, jitter, net.weights(), net.biases(), **kw)[2:]


class Renderer(nn.Module):
    def __init__(self, model, cfg, device=None, **kwargs):
        super().__init__()
        self._device = device
        self.depth_range = cfg['depth_range']
        self.n_max_network_queries = cfg['n_max_network_queries']   # kept for API parity; the fused kernel needs no chunking
        self.white_background = cfg['white_background']
        self.cfg = cfg
        self.model = model.to(device)
        self._z_cache = {}
        self.jitter_window = None   # (first ray, rays in the whole step) when this process renders a shard
        self.normal_window = None   # (validity of ALL rays of the step, first ray) for the normal term of a shard
        self.ray_distortion = False   # set by the trainer for a step whose training.ray_distortion_weight is not 0: out['ray_distortion']

    def forward(self, pixels, depth, camera_mat, world_mat, scale_mat, rendering_technique, add_noise=True,
                eval_=False, it=1000000, rays=None):
        if rendering_technique == 'nope_nerf':
            return self.nope_nerf(pixels, depth, camera_mat, world_mat, scale_mat, it=it, add_noise=add_noise, eval_=eval_, rays=rays)
        if rendering_technique == 'phong_renderer':
            return self.phong_renderer(pixels, camera_mat, world_mat, scale_mat, it=it)
        raise ValueError('unknown rendering technique %r' % (rendering_technique,))

    # ------------------------------------------------------------------------------------------------ z tables
    def _z_tables(self, n_samples, near, far, stratified, device):
        """Per-sample interval [lo_j, hi_j]; z_j = lo_j + (hi_j - lo_j) * u_j (reference rendering.py:95-96,184-190).
        Built once per configuration on the CPU (bit-identical to the reference's CPU arithmetic), then cached on the
        device; the kernel applies the jitter."""
        key = (n_samples, float(near), float(far), bool(stratified), str(device))
        hit = self._z_cache.get(key)
        if hit is None:
            rng = torch.tensor([near, far])
            z = torch.linspace(0., 1., steps=n_samples)
            z = rng[0] * (1. - z) + rng[1] * z
            if stratified:
                mid = .5 * (z[1:] + z[:-1])
                lo, hi = torch.cat([z[:1], mid]), torch.cat([mid, z[-1:]])
            else:
                lo = hi = z
            hit = (lo.contiguous().to(device), hi.contiguous().to(device))
            self._z_cache[key] = hit
        return hit

    def _unit_tables(self, n, device):
        """z_lo = 0, z_hi = 1 of n samples: with them the render kernels' z = z_lo + (z_hi - z_lo) * jitter is the jitter tensor bit for
        bit -- how the fine pass of hierarchical sampling hands over per-ray depths.  Cached per size."""
        key = ('unit', int(n), str(device))
        hit = self._z_cache.get(key)
        if hit is None:
            hit = (torch.zeros(n, device=device), torch.ones(n, device=device))
            self._z_cache[key] = hit
        return hit

    def _fine_draw(self, n_rays, n_fine, device):
        """xi (R, num_fine) in [0,1): the stratified offsets of the fine samples, drawn right after the jitter.  A data-parallel shard takes
        its rows of the whole step's draw, as for the jitter, so that every rank's generator ends where the single-process run's does."""
        if self.jitter_window is None:
            return torch.rand(n_rays, n_fine, device=device)
        lo, total = self.jitter_window
        from nnr import sampling
        return sampling.rand_rows(total * n_fine, lo * n_fine, n_rays * n_fine, device).view(n_rays, n_fine)

    # ------------------------------------------------------------------------------------------------ hot path
    def nope_nerf(self, pixels, depth, camera_mat, world_mat, scale_mat, add_noise=False, it=100000, eval_=False, rays=None):
        cfg = self.cfg
        batch_size, n_rays, _ = pixels.shape
        if batch_size != 1:
            raise NotImplementedError("batch size 1 is baked into the reference (rendering.py:86-87); so it is here")
        n_samples = cfg['num_points'] - cfg['outside_steps']
        device = pixels.device

        # --- rays (reference :54-87).  inv(S) inv(W) inv(K) stays inside autograd: pose / focal gradients flow here ---
        if rays is not None:
            # the trainer's fused front end (nnr.camera.step_rays) has generated them together with everything before them
            origin, ray, view, ray_norm, d_gt, object_mask = rays
        elif pixels.is_cuda:
            # one HIP launch (nnr_ray_setup_fwd; backward: nnr_ray_setup_bwd) for the three inverses, the unprojection,
            # norms, d_gt and the validity mask
            origin, ray, view, ray_norm, d_gt, object_mask = camera.ray_setup(
                pixels, depth, camera_mat, world_mat, scale_mat, bool(cfg['normalise_ray']), bool(cfg['use_ray_dir']))
        else:
            m = pixel_to_world_matrix(camera_mat, world_mat, scale_mat)[0]             # (4,4)
            cam = m[:3, 3]                                                              # camera centre
            pix_h = torch.cat([pixels[0], torch.ones(n_rays, 1, device=device)], dim=-1)   # (R,3) = (x', y', 1)
            ray = pix_h @ m[:3, :3].t()                                                 # pixels_world - camera_world
            ray_norm = ray.norm(2, -1)
            d_gt = (ray * depth[0]).norm(2, -1)                                         # |points_world - camera_world|
            if cfg['normalise_ray']:
                ray = ray / ray_norm.unsqueeze(-1)
            else:
                d_gt = d_gt / ray_norm
            object_mask = torch.isfinite(d_gt) & (d_gt != 0)                            # :73-87
            view = -ray if cfg['use_ray_dir'] else torch.ones_like(ray)                 # :104-105,194-195
            origin = cam.unsqueeze(0).expand(n_rays, 3)

        # --- per-ray sampling frame ---
        jitter = None
        if cfg['sample_option'] == 'ndc':                                           # :168-180
            if pixels.is_cuda and not camera_mat.requires_grad:       # one launch each way instead of ~25 + ~50 torch ops
                pts_o, pts_d = camera.ndc_rays(origin, ray, camera_mat, 1.0)
            else:                                                    # CPU stand-in; a focal that is being learned
                focal = torch.cat([camera_mat[:, 0, 0], camera_mat[:, 1, 1]])
                pts_o, pts_d = get_ndc_rays_fxfy(focal, 1.0, rays_o=origin, rays_d=ray)
            z_lo, z_hi = self._z_tables(n_samples, 0., 1., False, device)
        elif cfg['sample_option'] == 'uniform':                                     # :182-197
            pts_o, pts_d = origin, ray
            z_lo, z_hi = self._z_tables(n_samples, self.depth_range[0], self.depth_range[1], bool(add_noise), device)
            if add_noise:
                if self.jitter_window is None:
                    jitter = torch.rand(batch_size, n_rays, n_samples, device=device)   # same draw as the reference (:189)
                else:   # data-parallel shard: this rank's rows of the whole step's jitter tensor (model/training.py) -- drawn alone,
                        # O(rays of this rank): nnr.sampling.rand_rows reproduces torch.rand's values and its generator side effects
                    lo, total = self.jitter_window
                    if batch_size == 1 and torch.device(device).type == 'cuda':
                        from nnr import sampling
                        jitter = sampling.rand_rows(total * n_samples, lo * n_samples, n_rays * n_samples, device).view(1, n_rays, n_samples)
                    else:
                        jitter = torch.rand(batch_size, total, n_samples, device=device)[:, lo:lo + n_rays].contiguous()
        else:
            raise ValueError('unknown sample_option %r' % (cfg['sample_option'],))

        net = self.model
        kw = dict(hidden=net.hidden_dim, dist_alpha=bool(cfg['dist_alpha']), white_bg=bool(self.white_background),
                  relu_sigma=(net.occ_activation != 'softplus'),
                  bf16=(str(cfg.get('mfma_dtype', 'fp32')).lower() == 'bf16'))   # rendering.mfma_dtype: fp32 (default) | bf16
        n_fine = int(cfg.get('num_fine', 0) or 0)    # rendering.num_fine: hierarchical sampling, 0 / absent = off (nothing below changes)
        grid, grid_asked = None, False      # rendering.occupancy: the render's grid, and whether it has been asked for already
        if n_fine > 0:
            proposal = cfg.get('proposal', None) or 'render'      # rendering.proposal (absent = 'render'; ignored without num_fine)
            if proposal not in ('render', 'density'):
                raise ValueError("rendering.proposal: expected 'render' or 'density', got %r" % (proposal,))
            # rendering.occupancy.proposal (absent = false; ignored without num_fine, as rendering.proposal is): the proposal skips the coarse
            # samples the grid calls empty.  A setting of the render, not of the grid: it is no part of the grid's cache key
            sparse_proposal = bool((cfg.get('occupancy', None) or {}).get('proposal', False))
            if sparse_proposal and proposal != 'density':
                raise ValueError("rendering.occupancy.proposal: true needs rendering.proposal: 'density' (there is no sparse %r proposal)"
                                 % (proposal,))
            if not pixels.is_cuda:
                raise NotImplementedError("rendering.num_fine > 0 runs only on the GPU (HIP resampling kernel, nnr_resample.hip); there is no "
                                          "CPU hierarchical sampling -- set rendering.num_fine: 0 for CPU runs")
            # coarse pass (the inference forward: no stash, only alpha and z) -> nnr_resample -> the render proper at the sorted union of
            # the coarse depths and n_fine inverse-CDF samples of the coarse weights.  One network, trained at both sample sets; the
            # depths carry no gradient, pose / distortion gradients flow through pts_o / pts_d as before.
            # rendering.proposal: 'render' (default) = that pair of launches; 'density' = one launch of the fused proposal kernel
            # (nnr_propose_f16.hip through nnr.ops.propose): the coarse samples' density alone, always in the two-term fp16 products.
            xi = self._fine_draw(n_rays, n_fine, device) if (jitter is not None) else None   # after the jitter draw; else u at bin centres
            if proposal == 'density':
                pgrid = None
                if sparse_proposal:
                    # the grid the render below uses, asked for in front of the proposal (its sample count is known: the union's); inside
                    # nnr.frozen_field(occupancy=grid) -- pose refinement, gradients enabled -- that block's grid, the one render_rays uses
                    # there.  Where the grid is refused (one logged line) the dense proposal runs
                    grid, grid_asked = self._occupancy_grid(pixels, n_samples + n_fine, kw), True
                    pgrid = grid
                    if pgrid is None and not kw['bf16']:
                        pgrid = _nnr_ops.frozen_occupancy()
                pkw = dict(hidden=kw['hidden'], dist_alpha=kw['dist_alpha'], relu_sigma=kw['relu_sigma'])
                if pgrid is not None:      # nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1, through nnr.ops.propose_sparse
                    z_all = _nnr_ops.propose_sparse(pts_o, pts_d, z_lo, z_hi, jitter, xi, n_fine, pgrid, net.weights(), net.biases(), **pkw)
                else:
                    z_all = _nnr_ops.propose(pts_o, pts_d, z_lo, z_hi, jitter, xi, n_fine, net.weights(), net.biases(), **pkw)
                z_lo, z_hi = self._unit_tables(n_samples + n_fine, device)
                jitter = z_all
            else:      # today's path, as it was written
                with torch.no_grad():
                    _, _, alpha_c, z_c = nnr.render_rays(pts_o, pts_d, view, z_lo, z_hi, jitter, net.weights(), net.biases(), samples=True, **kw)
                z_lo, z_hi = self._unit_tables(n_samples + n_fine, device)      # z = 0 + (1 - 0) * jitter: the kernels take the depths as given
                jitter = _nnr_ops.resample(alpha_c, z_c, xi, n_fine)
        # the ray distortion of the compositing weights (training.ray_distortion_weight; nnr_ray_distortion.hip): on the training render only,
        # at depths normalised by the COARSE range, whatever num_fine added
        ray_distortion = None
        if self.ray_distortion and torch.is_grad_enabled() and not eval_:
            if not pixels.is_cuda:
                raise NotImplementedError("training.ray_distortion_weight != 0 runs only on the GPU (HIP kernels, nnr_ray_distortion.hip); there "
                                          "is no CPU ray distortion -- set training.ray_distortion_weight: 0 for CPU runs")
            if cfg['sample_option'] == 'ndc':
                ray_distortion = (0.0, 1.0)
            else:
                ray_distortion = (float(self.depth_range[0]), 1.0 / (float(self.depth_range[1]) - float(self.depth_range[0])))
        lazy_samples = not torch.is_grad_enabled()   # evaluation / visualisation: per-sample outputs only if somebody reads them
        if not grid_asked and cfg.get('occupancy', None) is not None:
            grid = self._occupancy_grid(pixels, int(z_lo.shape[0]), kw)
        if grid is not None:
            # rendering.occupancy: the sparse inference render (nnr_sparse_f16.hip), the samples in known-empty cells skipped; alpha / z_vals,
            # if somebody reads them, still come from the dense pass below.  rendering.occupancy.t_min (absent or 0: off; no default): early
            # ray termination, nnr_render_sparse_stop -- a setting of the render, not of the grid: it is no part of the grid's cache key
            rgb, dist_pred, _ = _nnr_ops.render_sparse(pts_o, pts_d, view, z_lo, z_hi, jitter, grid, net.weights(), net.biases(),
                                                       hidden=kw['hidden'], dist_alpha=kw['dist_alpha'], white_bg=kw['white_bg'],
                                                       relu_sigma=kw['relu_sigma'], t_min=float(cfg['occupancy'].get('t_min', None) or 0.0))
            alpha = z_val = None
        elif ray_distortion is not None:
            rgb, dist_pred, alpha, z_val, dloss = nnr.render_rays(pts_o, pts_d, view, z_lo, z_hi, jitter, net.weights(), net.biases(),
                                                                  samples=not lazy_samples, ray_distortion=ray_distortion, **kw)
            if dloss is None:
                raise RuntimeError("training.ray_distortion_weight != 0, but nothing the render depends on requires a gradient")
        else:
            rgb, dist_pred, alpha, z_val = nnr.render_rays(pts_o, pts_d, view, z_lo, z_hi, jitter, net.weights(), net.biases(),
                                                           samples=not lazy_samples, **kw)

        diff_norm = None
        if cfg['normal_loss'] and not eval_:
            diff_norm = self._normal_consistency(origin, ray, d_gt, object_mask, it)

        if eval_ and cfg['normalise_ray']:                                          # distance -> depth for evaluation (:150-154)
            dist_pred = dist_pred / ray_norm
            d_gt = d_gt / ray_norm
        return RenderOutput({
            'rgb': rgb.reshape(batch_size, -1, 3),
            'normal': diff_norm,
            **({'_samples': lambda: _forward_only_samples(pts_o, pts_d, view, z_lo, z_hi, jitter, net, kw)}
               if lazy_samples else {'z_vals': z_val, 'alpha': alpha}),
            # dense per-ray values + validity mask; 'depth_pred' / 'depth_gt' (masked) are derived lazily from these
            'dist_dense': dist_pred,
            'd_gt_dense': d_gt,
            'mask': object_mask,
            'ndc': cfg['sample_option'] == 'ndc',
            **({'ray_distortion': dloss} if ray_distortion is not None else {}),
        })

    # ------------------------------------------------------------------------------------------------ sparse inference render
    def frozen_occupancy_grid(self, device):
        """eval_pose.occupancy (model.Trainer_pose): the occupancy grid of this renderer's field for nnr.frozen_field(occupancy=grid), from the
        rendering.occupancy settings -- the same bounds rules, the same level (geometry.level_for_alpha), the same refusals other than
        "gradients are enabled" (None where the dense path has to run; at most 1024 samples per ray here).  Built anew on every call and
        not kept here: the caller owns it, and says the field is frozen."""
        cfg = self.cfg
        if cfg.get('occupancy', None) is None:
            raise ValueError("eval_pose.occupancy: true needs the rendering.occupancy settings (resolution, alpha_min; DESIGN.md section 15)")
        net = self.model
        kw = dict(dist_alpha=bool(cfg['dist_alpha']), relu_sigma=(net.occ_activation != 'softplus'),
                  bf16=(str(cfg.get('mfma_dtype', 'fp32')).lower() == 'bf16'))
        n_render = int(cfg['num_points']) + int(cfg.get('num_fine', 0) or 0)
        with torch.no_grad():
            return self._occupancy_grid(torch.empty(0, device=device), n_render, kw, frozen=True)

    def _occupancy_grid(self, pixels, n_render, kw, frozen=False):
        """rendering.occupancy: {resolution: N, alpha_min: A, dilate: 1, bounds: [lo, hi]} -> the occupancy grid of the sparse inference render
        (model.geometry.occupancy_grid), or None where the dense path has to run (one logged line per reason).  N cells per axis over
        `bounds` (two scalars or two triples; default: the cube of rendering.radius under sample_option 'uniform'; required under 'ndc', where
        the grid lives in the MLP's input space); a cell is empty where the raw density at its 8 corners stays below the level whose alpha at
        the coarse sample spacing is alpha_min (geometry.level_for_alpha; required: no default), `dilate` cells (default 1) around the others
        kept.  Built on first use and kept exactly as long as the packed weights it was built from are valid: the same parameter objects
        and no optimiser step since (nnr.ops.ParamsStamp)."""
        from . import geometry
        cfg = self.cfg
        occ = cfg['occupancy']
        why = None      # (n_render: the samples per ray of the render the grid is for)
        if torch.is_grad_enabled() and not frozen:
            why = "gradients are enabled (the sparse render is forward-only)"
        elif not pixels.is_cuda:
            why = "the tensors are not on the GPU"
        elif kw['bf16']:
            why = "rendering.mfma_dtype is bf16 (the sparse kernel has two-term fp16 products only)"
        elif frozen and n_render > 1024:
            why = "%d samples per ray (the frozen kernels take at most 1024)" % n_render
        elif not frozen and n_render > 256:
            why = "%d samples per ray (the sparse kernel takes at most 256)" % n_render
        if why is not None:
            seen = self.__dict__.setdefault('_occupancy_said', set())
            if why not in seen:
                seen.add(why)
                logging.getLogger(__name__).info("rendering.occupancy: dense render, %s", why)
            return None
        if 'alpha_min' not in occ or 'resolution' not in occ:
            raise ValueError("rendering.occupancy needs `resolution` and `alpha_min` (no defaults: DESIGN.md section 12)")
        bounds = occ.get('bounds', None)
        if bounds is None:
            if cfg['sample_option'] != 'uniform':
                raise ValueError("rendering.occupancy.bounds must be given under sample_option %r (default only under 'uniform': the cube of "
                                 "rendering.radius)" % (cfg['sample_option'],))
            bounds = [-float(cfg['radius']), float(cfg['radius'])]
        lo, hi = ([float(b)] * 3 if not isinstance(b, (list, tuple)) else [float(v) for v in b] for b in bounds)
        net = self.model
        w, b = net.weights(), net.biases()
        hit = self.__dict__.get('_occupancy_hit', None)
        key = (tuple(lo), tuple(hi), repr(occ.get('resolution')), float(occ['alpha_min']), int(occ.get('dilate', 1)), kw['dist_alpha'], kw['relu_sigma'])
        if not frozen and hit is not None and hit[0] == key and hit[1].matches(w, b):
            return hit[2]
        n_coarse = cfg['num_points'] - cfg['outside_steps']
        near, far = (0., 1.) if cfg['sample_option'] == 'ndc' else (float(self.depth_range[0]), float(self.depth_range[1]))
        delta = (far - near) / max(n_coarse - 1, 1) if kw['dist_alpha'] else None      # the coarse spacing: fine samples lie closer
        level = geometry.level_for_alpha(occ['alpha_min'], delta, 'relu' if kw['relu_sigma'] else 'softplus')
        res = occ['resolution']
        grid = geometry.occupancy_grid(self, lo, hi, int(res) if not isinstance(res, (list, tuple)) else tuple(res), level, int(occ.get('dilate', 1)))
        if frozen:      # (the caller's grid: no stamp -- the pose optimiser steps every iteration, and the field is frozen by declaration)
            return grid
        stamp = _nnr_ops.ParamsStamp(w, b)      # (after the build: density_volume packs the weights if need be)
        self.__dict__['_occupancy_hit'] = (key, stamp, grid)
        self.occupancy_builds = getattr(self, 'occupancy_builds', 0) + 1
        return grid

    def _normal_consistency(self, origin, ray, d_gt, mask, it):
        """|n(x) - n(x + eps)| at the surface points x the mono depth puts on the valid rays, n = normalised -d(sigma)/dx
        (reference rendering.py:76-93,133-141).  Stock autograd over the MLP's own parameters (OfficialStaticNerf.gradient); the
        perturbation draws torch.rand_like(surface_points) right after the jitter draw, as the reference does.  A data-parallel
        shard draws the whole step's perturbations and keeps the rows of its own valid rays, so every rank's generator stays where
        the single-process run leaves it."""
        surface = (origin + ray * d_gt.unsqueeze(-1))[mask]            # dists == d_i on the valid rays (:80-82,92)
        n = surface.shape[0]
        if self.normal_window is None:
            noise = torch.rand_like(surface)
        else:
            # data parallel: the rank draws the whole step's perturbations and keeps its rows, so that every rank's generator ends where
            # the single-process run's does (the reference draws rand_like(surface) over ALL valid rays).  The two int(...) below are
            # blocking device-to-host reads -- the only ones in a training step, taken only with rendering.normal_loss on AND more than
            # one rank; the surface[mask] boolean indexing above synchronises in the single-process path as well (it is the reference's
            # own expression).  Everything else in the step stays on the device (deferred NaN flag, device-side counts).
            valid_all, lo = self.normal_window
            first = int(valid_all[:lo].sum())
            noise = torch.rand(int(valid_all.sum()), 3, dtype=surface.dtype, device=surface.device)[first:first + n]
        neigh = surface + (noise - 0.5) * 0.01
        g = self.model.gradient(torch.cat([surface, neigh], dim=0), it)
        normals = g[:, 0, :] / (g[:, 0, :].norm(2, dim=1).unsqueeze(-1) + 10 ** (-5))
        return torch.norm(normals[:n] - normals[n:], dim=-1)

    # ------------------------------------------------------------------------------------------------ geometry visualisation
    def _t_table(self, n_steps, device):
        """torch.linspace(0, 1, n_steps) on the device (reference :327-329: built on the CPU, as there), cached per size.  The first use
        of a size copies from pinned memory without blocking, so that no call of phong_renderer synchronises with the device."""
        key = ('t', int(n_steps), str(device))
        hit = self._z_cache.get(key)
        if hit is None:
            hit = torch.linspace(0, 1, steps=n_steps).pin_memory().to(device, non_blocking=True)
            self._z_cache[key] = hit
        return hit

    def phong_renderer(self, pixels, camera_mat, world_mat, scale_mat, it):
        """Reference rendering.py:202-273 on the GPU: the depth search (ray_marching), the surface normals -d(raw)/dp / |.| and the
        diffuse shading with the light at the camera, plus the colour branch at the surface point.  The march runs in
        nnr_march_f16.hip, the normals through the training kernels (nnr.ops.density_grad), rgb_surf through nnr.ops.mlp_points; all
        three always use the two-term fp16 products (NNR_F_SPLIT3 | NNR_F_SPLIT2) whatever rendering.mfma_dtype or NNR_FP32_PRODUCTS
        select for the training step.  No device-to-host synchronisation: every ray is evaluated and masked afterwards.  GPU only."""
        if not pixels.is_cuda:
            raise NotImplementedError("phong_renderer runs only on the GPU (HIP march kernel, nnr_march_f16.hip); there is no CPU "
                                      "geometry renderer -- set training.vis_geo: False for CPU runs")
        batch_size, num_pixels, _ = pixels.shape
        if batch_size != 1:
            raise NotImplementedError("batch size 1 is baked into the reference (rendering.py:86-87); so it is here")
        rad = self.cfg['radius']
        net = self.model
        origin, ray, _, _, _, _ = camera.ray_setup(pixels, None, camera_mat, world_mat, scale_mat, True, True)
        light = origin[0] / origin[0].norm(2)                                            # camera_world[0,0], normalised (:218-220)
        self.model.eval()
        with torch.no_grad():
            d_i = self.ray_marching(origin.unsqueeze(0), ray.unsqueeze(0), self.model, n_secant_steps=8, n_steps=[512, 513],
                                    rad=rad)[0]
            mask_zero = d_i == 0
            mask_pred = torch.isfinite(d_i)                                              # get_mask (common.py)
            dists = torch.where(mask_pred, d_i, torch.ones_like(d_i)).masked_fill(mask_zero, 0.)
            obj = mask_pred & ~mask_zero
            points = origin + ray * dists.unsqueeze(-1)
            view = -ray
            g = _nnr_ops.density_grad(points, net.weights(), net.biases(), net.hidden_dim).neg()   # OfficialStaticNerf.gradient
            normals = g / g.norm(2, 1, keepdim=True)
            diffuse = (normals @ light.unsqueeze(1)).clamp_min(0).repeat(1, 3) * 0.7
            rgb = torch.where(obj.unsqueeze(-1), (0.3 + diffuse).clamp_max(1.0), torch.ones_like(points))
            rgb_s, _ = _nnr_ops.mlp_points(points, view, net.weights(), net.biases(), hidden=net.hidden_dim, split2=True)
            rgb_surf = torch.where(obj.unsqueeze(-1), rgb_s, torch.zeros_like(rgb_s))
        return {'rgb': rgb.reshape(batch_size, -1, 3), 'normal': None, 'rgb_surf': rgb_surf.reshape(batch_size, -1, 3)}

    def ray_marching(self, ray0, ray_direction, model, c=None, tau=0.5, n_steps=[128, 129], n_secant_steps=8,
                     depth_range=[0., 2.4], max_points=3500000, rad=1.0):
        """Reference rendering.py:277-386 (+ secant, :388-418) in one call of nnr.ops.ray_march: (B=1, R, 3) origins and unit
        directions -> d (1, R): the surface depth on a hit, inf on a miss, 0 where the first proposal is occupied.  Proposals from 0
        (depth_range[0] of the reference, which the CPU reference multiplies by (1 - t)) to the far root of the radius-`rad` sphere;
        tau is 0.5 as in the reference (which overwrites its argument).  One draw of torch's CPU generator, as the reference makes."""
        n = int(torch.randint(n_steps[0], n_steps[1], (1,)).item())
        if not ray0.is_cuda:
            raise NotImplementedError("ray_marching runs only on the GPU (HIP march kernel, nnr_march_f16.hip)")
        if ray0.shape[0] != 1:
            raise NotImplementedError("batch size 1 is baked into the reference (rendering.py:86-87); so it is here")
        if float(depth_range[0]) != 0.:
            raise NotImplementedError("the march kernel starts its proposals at 0 (the reference's default and the only value phong uses)")
        net = model
        d = _nnr_ops.ray_march(ray0[0], ray_direction[0], self._t_table(n, ray0.device), net.weights(), net.biases(),
                               hidden=net.hidden_dim, radius=float(rad), n_secant=int(n_secant_steps),
                               relu_sigma=(net.occ_activation != 'softplus'), dist_alpha=bool(net.dist_alpha))
        return d.unsqueeze(0)

    def secant(self, f_low, f_high, d_low, d_high, n_secant_steps, ray0_masked, ray_direction_masked, tau, it=0):
        """Reference rendering.py:388-418 on its own (phong_renderer runs these steps inside the march kernel): the same updates with
        torch.where instead of boolean-mask assignment, occ from OfficialStaticNerf.forward (the fused kernel on free-standing points).
        GPU only."""
        if not ray0_masked.is_cuda:
            raise NotImplementedError("secant runs only on the GPU (the fused MLP kernel); there is no CPU geometry renderer")
        d_low, d_high, f_low, f_high = (t.clone() for t in (d_low, d_high, f_low, f_high))
        d_pred = - f_low * (d_high - d_low) / (f_high - f_low) + d_low
        for _ in range(n_secant_steps):
            p_mid = ray0_masked + d_pred.unsqueeze(-1) * ray_direction_masked
            with torch.no_grad():
                f_mid = self.model(p_mid, batchwise=False, only_occupancy=True, it=it)[..., 0] - tau
            ind_low = f_mid < 0
            d_low = torch.where(ind_low, d_pred, d_low)
            f_low = torch.where(ind_low, f_mid, f_low)
            d_high = torch.where(ind_low, d_high, d_pred)
            f_high = torch.where(ind_low, f_high, f_mid)
            d_pred = - f_low * (d_high - d_low) / (f_high - f_low) + d_low
        return d_pred
