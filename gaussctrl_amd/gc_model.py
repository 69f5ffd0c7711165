"""GaussCtrlModel: drop-in for /root/reference/gaussctrl/gc_model.py (GaussCtrlModelConfig :39-50,
GaussCtrlModel.get_outputs :57-206, get_outputs_for_camera :208-221) on the HIP rasterizer.

Same contract: get_outputs(camera: Cameras[1]) -> {"rgb"[H,W,3], "depth"[H,W,1] | None,
"accumulation"[H,W,1]}; training -> random / configured background and no depth; eval -> rgb + depth +
accumulation from ONE fused compositing sweep (the reference sorts and rasterises twice, :174-202); returns a
background image when nothing is visible (:89-91,155-156); `self.xys` / `self.radii` are kept for the densification
callbacks and `self.xys.grad` is populated after backward (:159-160).  Parameter names / optimizer groups are
splatfacto's (`means, scales, quats, features_dc, features_rest, opacities`; groups xyz, features_dc, features_rest,
opacity, scaling, rotation -- /root/reference/gaussctrl/gc_config.py:58-87)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Union

import torch
from torch import nn

from . import gsplat_ops as ops
from .camera import camera_to_gsplat
from .ns_compat import HAVE_NERFSTUDIO, Cameras

if HAVE_NERFSTUDIO:  # the reference's bases (gc_model.py:39,52): SplatfactoModelConfig / SplatfactoModel
    from nerfstudio.models.splatfacto import SplatfactoModel as _ModelBase, SplatfactoModelConfig as _ModelConfigBase  # type: ignore
else:
    _ModelBase = nn.Module

    @dataclass
    class _ModelConfigBase:
        """the SplatfactoModelConfig fields get_outputs / the loss / the culling callback read [recall nerfstudio 1.0.0]"""
        sh_degree: int = 3
        sh_degree_interval: int = 1000
        background_color: str = "random"
        ssim_lambda: float = 0.2
        cull_alpha_thresh: float = 0.1
        cull_scale_thresh: float = 0.5
        refine_every: int = 100
        reset_alpha_every: int = 30
        stop_split_at: int = 15000
        continue_cull_post_densification: bool = True
        # the rest of splatfacto's refinement schedule (gaussctrl_amd/refine.py reads them; splatfacto's defaults)
        warmup_length: int = 500
        densify_grad_thresh: float = 0.0002
        densify_size_thresh: float = 0.01
        n_split_samples: int = 2
        cull_screen_size: float = 0.15
        split_screen_size: float = 0.05
        stop_screen_size_at: int = 4000

        def setup(self, **kw):
            return self._target(self, **kw)


@dataclass
class GaussCtrlModelConfig(_ModelConfigBase):
    """gc_model.py:39-50: the four fields the reference adds (never read: it has no get_loss_dict override)."""
    _target: type = field(default_factory=lambda: GaussCtrlModel)
    use_lpips: bool = True
    use_l1: bool = True
    patch_size: int = 32
    lpips_loss_mult: float = 1.0
    # --- addition of this implementation (the name later splatfacto versions use)
    output_depth_during_training: bool = False    # True: get_outputs in training mode also returns "depth" [H,W,1], differentiable
                                                  # (ops.RenderAux.depth_grad); False: no depth while training, as the reference
    refine_on_device: bool = False                # True (stand-alone model): get_training_callbacks returns [StepCallback, RefineCallback] --
                                                  # splatfacto's whole refinement (statistics, split / duplicate, cull, opacity reset) on the
                                                  # HIP kernels of csrc/train_refine.hip; False: the callbacks as before (CullCallback)
    rasterize_mode: str = "classic"               # "classic": gsplat 0.1.3's rasterizer, the reference's (every projected covariance gets +0.3 on
                                                  # its diagonal, opacities untouched); "antialiased": later splatfacto's mode of that name -- each
                                                  # view also multiplies the opacity by sqrt(det(cov2d) / det(cov2d + 0.3 I)) (ops.RenderAux.antialiased),
                                                  # for scenes trained that way or rendered below their training resolution.  Declared here, so the
                                                  # field exists (and defaults to the reference's behaviour) with and without nerfstudio
    use_absgrad: bool = False                     # True: absgrad densification (AbsGS; later splatfacto's switch of that name) -- the training
                                                  # backward also sums |dL_p/dxy| per pixel (ops.RenderAux.absgrad -> GaussCtrlModel.xys_absgrad) and
                                                  # the on-device refinement accumulates ITS norm instead of the signed gradient's, so a large splat
                                                  # whose pixels pull in opposite directions is still split.  densify_grad_thresh keeps its default
                                                  # 0.0002: later splatfacto pairs absgrad with about 0.0008 (a figure recalled from nerfstudio 1.1,
                                                  # not checked against its source) -- raise it yourself, absolute sums are several times larger.
                                                  # Declared here like rasterize_mode; under nerfstudio only the property is offered, the inherited
                                                  # splatfacto callbacks keep reading xys_grad
    densify_strategy: str = "default"             # "default": the refinement above (CullCallback, or RefineCallback with refine_on_device);
                                                  # "mcmc": the strategy of 3DGS-MCMC (gsplat 1.x MCMCStrategy) on the kernels of
                                                  # csrc/train_mcmc.hip -- the stand-alone model's callbacks become [StepCallback, McmcCallback]
                                                  # whatever refine_on_device says, and its loss gains the two regularisers below.  The formulas
                                                  # are recalled from the paper and gsplat 1.x, not checked against their source
                                                  # (include/gaussctrl_mcmc.h is the contract).  Under nerfstudio the fields exist and are
                                                  # validated; the inherited callbacks and loss stay
    mcmc_cap_max: int = 1_000_000                 # the scene never grows past this many Gaussians
    mcmc_noise_lr: float = 5e5                    # the perturbation of the means is scaled by (xyz learning rate) * mcmc_noise_lr
    mcmc_min_opacity: float = 0.005               # sigmoid(opacity) <= this: dead, relocated at the next refinement step
    mcmc_refine_start_iter: int = 500             # refinement steps: start < step < stop and step % every == 0.  A GaussCtrl run starts at
    mcmc_refine_stop_iter: int = 25_000           # step 30000: raise mcmc_refine_stop_iter for relocation / growth to act there
    mcmc_refine_every: int = 100
    mcmc_opacity_reg: float = 0.01                # loss += mcmc_opacity_reg * mean(sigmoid(opacities))
    mcmc_scale_reg: float = 0.01                  # loss += mcmc_scale_reg * mean(exp(scales))
    use_bilateral_grid: bool = False              # True (stand-alone model, one GPU): every training view owns a learnable 3D grid of 3x4 colour
                                                  # transforms (later splatfacto's switch of that name; gaussctrl_amd/bilagrid.py on the kernels of
                                                  # csrc/train_bilagrid.hip).  In training mode the loss is taken on the render sliced through the
                                                  # view's grid at (x, y, luma), so exposure / white-balance drift between the edited views lands in
                                                  # the grids, not in the Gaussians; outputs, metrics and evaluation never see the grid.  The model
                                                  # then needs num_train_data, owns the parameter `bilateral_grid` and the group "bilateral_grid".
                                                  # The formulas are recalled from the paper and gsplat 1.x, not checked against their source
                                                  # (include/gaussctrl_bilagrid.h is the contract).  Under nerfstudio the fields exist and are
                                                  # validated; the inherited loss stays
    bilateral_grid_shape: tuple = (16, 16, 8)     # (GW, GH, L): vertices along x, y and luma; each at least 2
    bilagrid_tv_mult: float = 10.0                # loss += bilagrid_tv_mult * (total variation of all grids)   [gsplat's value, as recalled]
    bilagrid_lr: float = 2e-3                     # Adam learning rate of the group "bilateral_grid" (eps 1e-15)   [gsplat's value, as recalled]
    camera_optimizer_mode: str = "off"            # "off": constant poses, the reference's behaviour; "SO3xR3" (stand-alone model, one GPU, gradients
                                                  # through autograd): every training view owns a 6-vector (tau, omega) of the parameter
                                                  # `pose_adjustment`, group "camera_opt"; in training mode the view named by
                                                  # camera.metadata["cam_idx"] is rendered from c2w @ [exp(omega) | tau] and the renderer's view-matrix
                                                  # gradient (ops.RenderAux.pose_grad, include/gaussctrl_pose.h) reaches the row
                                                  # (gaussctrl_amd/camera_opt.py).  get_outputs_for_camera[s], render_reverse, metrics and evaluation
                                                  # never see the adjustment.  Later splatfacto's camera_optimizer, conventions as recalled.  Under
                                                  # nerfstudio the fields exist and are validated; the inherited behaviour stays
    camera_opt_lr: Optional[float] = None         # None: the group "camera_opt" follows the optimizer table (the reference's 1e-3 -> 5e-5 schedule);
                                                  # a number: constant Adam learning rate of the group (eps 1e-15), as bilagrid_lr
    camera_opt_trans_l2_penalty: float = 1e-2     # loss += this * mean |tau|      [nerfstudio's default, as recalled]
    camera_opt_rot_l2_penalty: float = 1e-3       # loss += this * mean |omega|    [nerfstudio's default, as recalled]
    distortion_loss_mult: float = 0.0             # 0: off, the reference's behaviour.  > 0: in training mode get_outputs also returns
                                                  # "distortion" [H,W,1], per pixel the weighted spread in depth of the splats composited there
                                                  # (the Mip-NeRF 360 / 2DGS regulariser against floaters; ops.RenderAux.distort on the kernels of
                                                  # csrc/raster_distort.hip), get_loss_dict adds "distortion_loss" = this * its mean and
                                                  # get_metrics_dict "distortion".  Evaluation, get_outputs_for_camera[s] and render_reverse never
                                                  # compute it.  The formulas are recalled from the papers and gsplat 1.x, not checked against their
                                                  # source (include/ext/gaussctrl_distort.h is the contract)
    distortion_depth_map: str = "linear"          # "linear": t = z, the camera-space depth; "ndc": t = far (z - near) / ((far - near) z), which
                                                  # weighs the spread near the camera more
    distortion_near: float = 0.2                  # the two planes of "ndc" (0 < near < far); "linear" does not read them
    distortion_far: float = 100.0

    def __post_init__(self):
        parent = getattr(super(), "__post_init__", None)
        if parent is not None:
            parent()
        _antialiased(self.rasterize_mode)
        _mcmc(self.densify_strategy)
        _bilagrid(self)
        _camera_opt(self)
        _distortion(self)


def _distortion(cfg) -> bool:
    """distortion_loss_mult > 0; a depth map that is not one of the two names is a ValueError (as are, under "ndc", planes without
    0 < near < far, and a negative multiplier)"""
    from .gsplat_ops import DISTORT_DEPTH_MAPS
    name = getattr(cfg, "distortion_depth_map", "linear")
    if name not in DISTORT_DEPTH_MAPS:
        raise ValueError(f"distortion_depth_map must be one of {DISTORT_DEPTH_MAPS}, got {name!r}")
    mult = float(getattr(cfg, "distortion_loss_mult", 0.0))
    if not mult >= 0:
        raise ValueError(f"distortion_loss_mult must be >= 0, got {mult!r}")
    if name == "ndc" and not 0 < float(cfg.distortion_near) < float(cfg.distortion_far) < float("inf"):
        raise ValueError(f"distortion_depth_map 'ndc' needs 0 < distortion_near < distortion_far, got {cfg.distortion_near!r}, {cfg.distortion_far!r}")
    return mult > 0


RASTERIZE_MODES = ("classic", "antialiased")


def _antialiased(mode) -> bool:
    """rasterize_mode -> RenderAux.antialiased; anything but the two names is a ValueError"""
    if mode not in RASTERIZE_MODES:
        raise ValueError(f"rasterize_mode must be one of {RASTERIZE_MODES}, got {mode!r}")
    return mode == "antialiased"


DENSIFY_STRATEGIES = ("default", "mcmc")


def _mcmc(strategy) -> bool:
    """densify_strategy -> is it "mcmc"; anything but the two names is a ValueError"""
    if strategy not in DENSIFY_STRATEGIES:
        raise ValueError(f"densify_strategy must be one of {DENSIFY_STRATEGIES}, got {strategy!r}")
    return strategy == "mcmc"


def _bilagrid(config) -> bool:
    """use_bilateral_grid with its three fields checked; a wrong type or range is a ValueError"""
    from .bilagrid import check_shape
    if not isinstance(getattr(config, "use_bilateral_grid", False), bool):
        raise ValueError(f"use_bilateral_grid must be a bool, got {config.use_bilateral_grid!r}")
    check_shape(getattr(config, "bilateral_grid_shape", (16, 16, 8)))
    for name in ("bilagrid_tv_mult", "bilagrid_lr"):
        v = getattr(config, name, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0 or v == float("inf") or (name == "bilagrid_lr" and v == 0):
            raise ValueError(f"{name} must be a finite {'positive' if name == 'bilagrid_lr' else 'non-negative'} number, got {v!r}")
    return bool(getattr(config, "use_bilateral_grid", False))


def _camera_opt(config) -> bool:
    """camera_optimizer_mode with its three numbers checked; a wrong name, type or range is a ValueError"""
    from .camera_opt import check_config
    return check_config(config)


class GaussCtrlModel(_ModelBase):
    """Under nerfstudio: a SplatfactoModel whose get_outputs / get_outputs_for_camera / loss run on the HIP kernels (parameters,
    densification callbacks, checkpoint keys and param groups are splatfacto's own).  Stand-alone: the same methods on an
    nn.Module that holds the six splatfacto parameter tensors."""
    config: GaussCtrlModelConfig

    def __init__(self, config: GaussCtrlModelConfig, *args, params: Optional[Dict[str, torch.Tensor]] = None, num_points: int = 0,
                 device="cuda", **kwargs):
        if HAVE_NERFSTUDIO:
            super().__init__(config, *args, **kwargs)         # SplatfactoModel.populate_modules creates the parameters
            self._aux = ops.RenderAux()
            return
        super().__init__()
        self.config = config
        k = (config.sh_degree + 1) ** 2 - 1
        if params is None:
            params = {"means": torch.zeros(num_points, 3), "scales": torch.zeros(num_points, 3),
                      "quats": torch.zeros(num_points, 4), "opacities": torch.zeros(num_points, 1),
                      "features_dc": torch.zeros(num_points, 3), "features_rest": torch.zeros(num_points, k, 3)}
        for name in ("means", "scales", "quats", "features_dc", "features_rest", "opacities"):
            setattr(self, name, nn.Parameter(torch.as_tensor(params[name], dtype=torch.float32).to(device).contiguous()))
        self.step = 30000                        # a loaded splatfacto checkpoint starts here (gc_trainer.py:75)
        self.crop_box = None
        self.background_color = torch.zeros(3)
        self.xys = None
        self.radii = None
        self.last_size = None
        self._aux = ops.RenderAux()
        if _bilagrid(config):
            # one grid per training view, identity at the start: a parameter, so it is in state_dict and in its own group
            from .bilagrid import identity_grids
            n = kwargs.get("num_train_data")
            if isinstance(n, bool) or not isinstance(n, int) or n < 1:
                raise ValueError(f"use_bilateral_grid needs num_train_data, the number of training views (a positive integer), got {n!r}")
            self.bilateral_grid = nn.Parameter(identity_grids(n, *config.bilateral_grid_shape, device=device))
        if _camera_opt(config):
            # one (tau, omega) row per training view, zero at the start: a parameter, so it is in state_dict and in its own group
            n = kwargs.get("num_train_data")
            if isinstance(n, bool) or not isinstance(n, int) or n < 1:
                raise ValueError(f"camera_optimizer_mode 'SO3xR3' needs num_train_data, the number of training views (a positive integer), got {n!r}")
            self.pose_adjustment = nn.Parameter(torch.zeros(n, 6, dtype=torch.float32, device=device))

    @property
    def device(self):
        return self.means.device

    @property
    def num_points(self):
        return self.means.shape[0]

    def set_crop(self, crop_box):
        self.crop_box = crop_box

    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        if HAVE_NERFSTUDIO:
            return super().get_param_groups()
        groups = {"xyz": [self.means], "features_dc": [self.features_dc], "features_rest": [self.features_rest],
                  "opacity": [self.opacities], "scaling": [self.scales], "rotation": [self.quats]}
        if getattr(self, "bilateral_grid", None) is not None:
            groups["bilateral_grid"] = [self.bilateral_grid]
        if getattr(self, "pose_adjustment", None) is not None:
            groups["camera_opt"] = [self.pose_adjustment]
        return groups

    def get_training_callbacks(self, training_callback_attributes):
        """SplatfactoModel's callbacks (step bookkeeping, after_train, refinement_after) under nerfstudio; stand-alone: the
        part of refinement_after that still acts after step 30000 (> stop_split_at = 15000): opacity / scale culling every
        `refine_every` steps [recall nerfstudio 1.0.0 splatfacto.py; SURVEY.md 3.5].  With config.refine_on_device the stand-alone model
        runs all of splatfacto's refinement on the device instead (gc_trainer.RefineCallback, which also covers that cull); under nerfstudio
        the inherited callbacks stay whatever the switch says.  With config.densify_strategy = "mcmc" the stand-alone model returns
        [StepCallback, McmcCallback] (gaussctrl_amd/mcmc.py), whatever refine_on_device says."""
        if HAVE_NERFSTUDIO:
            return super().get_training_callbacks(training_callback_attributes)
        from .gc_trainer import CullCallback, McmcCallback, RefineCallback, StepCallback
        if _mcmc(getattr(self.config, "densify_strategy", "default")):       # (checked again: the field may have been assigned)
            return [StepCallback(self), McmcCallback(self, training_callback_attributes.optimizers)]
        if getattr(self.config, "refine_on_device", False):
            dm = getattr(getattr(training_callback_attributes, "pipeline", None), "datamanager", None)
            n_train = len(getattr(dm, "train_data", None) or ())
            return [StepCallback(self), RefineCallback(self, training_callback_attributes.optimizers, n_train)]
        return [StepCallback(self), CullCallback(self, training_callback_attributes.optimizers)]

    # ------------------------------------------------------------------------------------ gc_model.py:57-206
    def get_outputs(self, camera: Cameras) -> Dict[str, Union[torch.Tensor, List]]:
        if not isinstance(camera, Cameras):
            print("Called get_outputs with not a camera")
            return {}
        assert camera.shape[0] == 1, "Only one camera at a time"
        dev = self.device
        if self.training:                                                       # :72-81
            bc = self.config.background_color
            background = (torch.rand(3, device=dev) if bc == "random" else torch.ones(3, device=dev) if bc == "white"
                          else torch.zeros(3, device=dev) if bc == "black" else self.background_color.to(dev))
            if bc == "random" and getattr(self, "background_override", None) is not None:
                background = self.background_override.to(dev)       # multi-GPU train_mode "parity": the colour rank 0 drew (GaussCtrlPipeline._sync_view)
        else:
            background = self.background_color.to(dev)
        W, H = int(camera.width.reshape(-1)[0]), int(camera.height.reshape(-1)[0])
        p = [self.means, self.scales, self.quats, self.opacities, self.features_dc, self.features_rest]
        if self.crop_box is not None and not self.training:                     # :88-93,123-136
            crop_ids = self.crop_box.within(self.means).squeeze()
            if crop_ids.sum() == 0:
                return {"rgb": background.repeat(H, W, 1)}
            p = [t[crop_ids] for t in p]
        c2w = camera.camera_to_worlds[0].detach().cpu().numpy()
        pose = getattr(self, "pose_adjustment", None) if (not HAVE_NERFSTUDIO and self.training) else None
        pose_row = None
        if pose is not None:
            # camera_optimizer_mode "SO3xR3": this view's pose, adjusted by its row (composed in float64 on the host; a zero row changes no bit)
            from . import camera_opt
            camera_opt.refuse_unsupported(self.config, train_mode="throughput" if getattr(self, "grad_into", None) is not None else "single",
                                          crop_in_training=self.crop_box is not None)
            pose_row = pose[camera_opt.check_view(camera, pose.shape[0])]
            c2w_plain, c2w = c2w, camera_opt.adjusted_c2w(c2w, pose_row)
        cam = camera_to_gsplat(c2w, float(camera.fx.reshape(-1)[0]),
                               float(camera.fy.reshape(-1)[0]), float(camera.cx.reshape(-1)[0]),
                               float(camera.cy.reshape(-1)[0]), W, H)        # :97-121 on the host
        self.last_size = (H, W)
        # :162-169: SH of degree n (+0.5, clamp) when config.sh_degree > 0, else sigmoid(features_dc) (encoded as n = -1)
        n = min(self.step // self.config.sh_degree_interval, self.config.sh_degree) if self.config.sh_degree > 0 else -1
        aux = self._aux = ops.RenderAux()
        aux.antialiased = _antialiased(getattr(self.config, "rasterize_mode", "classic"))      # (checked again: the field may have been assigned)
        if self.training and getattr(self, "grad_into", None) is not None and self.crop_box is None:
            # the fused backward writes the six leaf gradients straight into the caller's buffers (dist.FlatGrads: ONE flat allocation that
            # RCCL reduces in place) and autograd gets None for them: GaussCtrlPipeline.train_iteration, train_mode "throughput"
            aux.grad_into, aux.grad_accumulate = self.grad_into, False
        train_depth = bool(self.training and getattr(self.config, "output_depth_during_training", False))
        aux.depth_grad = train_depth
        aux.absgrad = bool(self.training and getattr(self.config, "use_absgrad", False))
        want_depth = train_depth or not self.training
        if self.training and getattr(self.config, "distortion_loss_mult", 0.0) > 0:      # the render also leaves aux.distort_map (the other
            # fields were validated in __post_init__; the operator layer and the entry points check the map name and the planes again)
            aux.distort, aux.distort_depth_map = True, self.config.distortion_depth_map
            aux.distort_near, aux.distort_far = float(self.config.distortion_near), float(self.config.distortion_far)
        if pose_row is not None and torch.is_grad_enabled() and pose_row.requires_grad:
            aux.pose_grad = True             # the projection backward also leaves aux.viewmat_grad, which the link chains to the row
            p[0] = camera_opt.link(p[0], pose_row, aux, c2w_plain)
        rgb, alpha, depth = ops.render_view(*p, cam, background, want_depth, n, aux)
        self.xys, self.radii = aux.xys, aux.radii
        if aux.M == 0:                                                          # :155-156
            return {"rgb": background.repeat(H, W, 1)}
        depth_im = depth[..., None] if want_depth else None
        outputs = {"rgb": rgb, "depth": depth_im, "accumulation": alpha[..., None]}
        if aux.distort_map is not None:
            outputs["distortion"] = aux.distort_map[..., None]
        return outputs

    forward = get_outputs

    if HAVE_NERFSTUDIO:
        def cull_gaussians(self, *args, **kwargs):
            """SplatfactoModel.cull_gaussians + a record of the row mask it applied: train_mode "sharded" prunes its 1 / N optimizer-state
            slices with it (GaussCtrlPipeline._sharded_adam), as splatfacto's own remove_from_all_optim does for the replicated Adam."""
            culls = super().cull_gaussians(*args, **kwargs)
            if torch.is_tensor(culls):
                self._cull_keep = ~culls
            return culls

    @property
    def xys_grad(self):
        """gradient of the loss w.r.t. the projected centres (what splatfacto's after_train reads as xys.grad)."""
        return self._aux.xys_grad

    @property
    def xys_absgrad(self):
        """sum over pixels of |dL_p/dxy| of the last training backward (config.use_absgrad; None without it or before the backward)."""
        return self._aux.xys_absgrad

    @torch.no_grad()
    def get_outputs_for_camera(self, camera: Cameras, obb_box=None) -> Dict[str, torch.Tensor]:    # :208-221
        assert camera is not None, "must provide camera to gaussian model"
        self.set_crop(obb_box)
        self.training = False
        outs = self.get_outputs(camera.to(self.device))
        self.training = True
        return outs

    @torch.no_grad()
    def get_outputs_for_cameras(self, cameras: List[Cameras], obb_box=None) -> List[Dict[str, torch.Tensor]]:
        """get_outputs_for_camera for a LIST of cameras of this scene through ONE batched launch set (ops.render_views: the parameter
        record is read once per batch, the sort / binning / compositing kernels run with the view as a grid dimension).  The reference has
        no such call -- render_reverse asks for one camera at a time (gc_pipeline.py:124-130); per view the outputs are bit-identical to
        get_outputs_for_camera.  Falls back to it when a crop box is set or the cameras differ in size."""
        cams = [c.to(self.device) for c in cameras]
        sizes = {(int(c.width.reshape(-1)[0]), int(c.height.reshape(-1)[0])) for c in cams}
        if obb_box is not None or len(cams) < 2 or len(sizes) != 1 or max(sizes.pop()) > 255 * 16:
            return [self.get_outputs_for_camera(c, obb_box) for c in cameras]
        self.set_crop(None)
        W, H = int(cams[0].width.reshape(-1)[0]), int(cams[0].height.reshape(-1)[0])
        gcams = [camera_to_gsplat(c.camera_to_worlds[0].detach().cpu().numpy(), float(c.fx.reshape(-1)[0]), float(c.fy.reshape(-1)[0]),
                                  float(c.cx.reshape(-1)[0]), float(c.cy.reshape(-1)[0]), W, H) for c in cams]
        background = self.background_color.to(self.device)
        n = min(self.step // self.config.sh_degree_interval, self.config.sh_degree) if self.config.sh_degree > 0 else -1
        aux = self._aux = ops.RenderAux()
        aux.antialiased = _antialiased(getattr(self.config, "rasterize_mode", "classic"))
        rgb, alpha, depth = ops.render_views(self.means, self.scales, self.quats, self.opacities, self.features_dc, self.features_rest,
                                             gcams, background, True, n, aux)
        self.last_size = (H, W)
        cnt = aux.M[0].cpu()
        outs = []
        for k in range(len(cams)):
            if int(cnt[k]) == 0:                                                # :155-156
                outs.append({"rgb": background.repeat(H, W, 1)})
            else:
                outs.append({"rgb": rgb[k], "depth": depth[k][..., None], "accumulation": alpha[k][..., None]})
        return outs

    # ------------------------------------------------------------------------------------ inherited splatfacto loss
    def get_metrics_dict(self, outputs, batch) -> Dict[str, torch.Tensor]:
        gt = batch["image"].to(self.device)
        mse = ((outputs["rgb"] - gt) ** 2).mean()
        metrics = {"psnr": -10.0 * torch.log10(mse.clamp_min(1e-12)), "gaussian_count": torch.tensor(self.num_points)}
        pose = getattr(self, "pose_adjustment", None) if not HAVE_NERFSTUDIO else None
        if pose is not None:             # camera_optimizer_mode "SO3xR3": how far the poses have moved, mean over the views
            metrics["camera_opt_translation"] = pose.detach()[:, :3].norm(dim=-1).mean()
            metrics["camera_opt_rotation"] = pose.detach()[:, 3:].norm(dim=-1).mean()
        if outputs.get("distortion") is not None:        # distortion_loss_mult > 0, training mode: the mean of the map
            metrics["distortion"] = outputs["distortion"].detach().mean()
        return metrics

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, torch.Tensor]:
        """SplatfactoModel.get_loss_dict [recall, SURVEY 8a/A8]: (1-l)*L1 + l*(1-SSIM), l = 0.2.  The stand-alone model with
        config.densify_strategy = "mcmc" adds the strategy's two regularisers (plain torch: two reductions over N, not the hot path).
        The stand-alone model with config.use_bilateral_grid, in training mode, takes the main loss on the render sliced through the grid
        of batch["image_idx"] and adds "tv_loss"; outputs["rgb"] itself, the metrics and everything at evaluation stay un-gridded.
        With config.camera_optimizer_mode = "SO3xR3" it adds, in training mode, "camera_opt_regularizer" (camera_opt.regularizer).
        With config.distortion_loss_mult > 0 it adds, in training mode, "distortion_loss" = mult * mean of outputs["distortion"]."""
        from .train_ops import l1_ssim_loss
        gt = batch["image"].to(self.device)
        grid = getattr(self, "bilateral_grid", None) if (not HAVE_NERFSTUDIO and self.training) else None
        if grid is not None:
            from .bilagrid import bilagrid_apply, bilagrid_tv_loss, check_view
            view = check_view(batch["image_idx"], grid.shape[0])
            pred = bilagrid_apply(grid, outputs["rgb"][None], [view])[0]
            loss = {"main_loss": l1_ssim_loss(pred, gt, self.config.ssim_lambda),
                    "tv_loss": self.config.bilagrid_tv_mult * bilagrid_tv_loss(grid)}
        else:
            loss = {"main_loss": l1_ssim_loss(outputs["rgb"], gt, self.config.ssim_lambda)}
        if not HAVE_NERFSTUDIO and _mcmc(getattr(self.config, "densify_strategy", "default")):
            loss["opacity_reg"] = self.config.mcmc_opacity_reg * torch.sigmoid(self.opacities).mean()
            loss["scale_reg"] = self.config.mcmc_scale_reg * torch.exp(self.scales).mean()
        pose = getattr(self, "pose_adjustment", None) if (not HAVE_NERFSTUDIO and self.training) else None
        if pose is not None:             # camera_optimizer_mode "SO3xR3": keep the adjustments small (plain torch over [V, 6])
            from .camera_opt import regularizer
            loss["camera_opt_regularizer"] = regularizer(pose, self.config.camera_opt_trans_l2_penalty, self.config.camera_opt_rot_l2_penalty)
        if outputs.get("distortion") is not None:        # distortion_loss_mult > 0, training mode (get_outputs leaves no key otherwise)
            loss["distortion_loss"] = self.config.distortion_loss_mult * outputs["distortion"].mean()
        return loss
