"""GPU test of depth supervision through the model and the pipeline: GaussCtrlModelConfig.output_depth_during_training and
GaussCtrlPipelineConfig.depth_loss_mult.

The stand-alone model part renders N = 3000 Gaussians at 72 x 40 (scene (a) of test_raster_depth_gpu.py).  The pipeline part renders the
same Gaussians at 64 x 64: render_reverse DDIM-inverts every render through the UNet, whose three stride-2 levels and exact x2 upsampling
need latents that are a multiple of 8, i.e. images that are a multiple of 64.  Seeds: syn.make_gaussians 4, syn.make_cameras(3, seed=12);
on the CPU the oracle in float32 and in float64 agrees on final_index, on the depth == 1000 mask and on the sorted lists for all three
cameras, before and after the 0.02 shift of the means, so the _grad_close comparison below sits on no knife edge."""
import numpy as np
import pytest
import torch

from gaussctrl_amd import synthetic as syn
from test_raster_gpu import _grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_model_and_pipeline_depth_supervision():
    from oracle import raster_torch as rt
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline, GaussCtrlPipelineConfig, SimpleDataManager
    from gaussctrl_amd.ns_compat import Cameras
    P = syn.make_gaussians(3000, seed=4, scale_mean=0.05)
    c2ws = syn.make_cameras(3, seed=12)
    # ---- the model switch, 72 x 40
    cams = Cameras(c2ws, 60.0, 59.4, 37.3, 17.9, 72, 40)
    model = GaussCtrlModel(GaussCtrlModelConfig(background_color="black"), params=P, device=DEV)
    assert model.training and model.config.output_depth_during_training is False
    assert model.get_outputs(cams[0])["depth"] is None
    model.config.output_depth_during_training = True
    out = model.get_outputs(cams[0])
    assert out["depth"].shape == (40, 72, 1) and out["depth"].requires_grad
    ev = model.get_outputs_for_camera(cams[0])
    assert torch.equal(ev["depth"], out["depth"].detach()) and not ev["depth"].requires_grad
    model.config.output_depth_during_training = False
    # ---- the pipeline, 64 x 64
    H = W = 64
    K = dict(fx=60.0, fy=60.0, cx=32.0, cy=32.0)
    cams = Cameras(c2ws, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    model = GaussCtrlModel(GaussCtrlModelConfig(background_color="black"), params=P, device=DEV)
    cfg = GaussCtrlPipelineConfig(edit_prompt="a polar bear", reverse_prompt="a bear", chunk_size=3, num_inference_steps=2, dtype="f16",
                                  synthetic_weights=True, depth_loss_mult=0.5)
    pipe = GaussCtrlPipeline(cfg, DEV, datamanager=SimpleDataManager(cams), model=model)
    dm = pipe.datamanager
    with pytest.raises(RuntimeError, match="depth_image"):       # no stored depth yet: a clear error, not a silent rgb-only loss
        pipe.get_train_loss_dict(0)
    pipe.render_reverse([0, 1, 2])
    for t in dm.train_data:
        t["image"] = t["unedited_image"].clone()                 # train against the renders themselves: no diffusion edit needed here
    VIEW = 2                                                      # (24 % of this view is empty: the sentinel mask matters)
    dm._pop_view = lambda: VIEW                                   # the test decides which view a step draws
    outs, loss_dict, _ = pipe.get_train_loss_dict(0)
    assert set(loss_dict) == {"main_loss", "depth_loss"} and outs["depth"].requires_grad
    assert model.config.output_depth_during_training is False     # switched on for the call only
    assert float(loss_dict["depth_loss"]) <= 1e-5                 # the training render against the eval render of the same parameters
    fwd = -np.stack([c[:3, 2] for c in c2ws]).mean(0); fwd /= np.linalg.norm(fwd)
    shift = (0.02 * fwd).astype(np.float32)
    with torch.no_grad():
        model.means += torch.tensor(shift, device=DEV)
    _, loss_dict, _ = pipe.get_train_loss_dict(1)
    assert float(loss_dict["depth_loss"]) > 0
    for p_ in model.parameters():
        p_.grad = None
    pipe.train_forward_backward(2)
    total = model.means.grad.detach().clone()
    pipe.config.depth_loss_mult = 0.0
    for p_ in model.parameters():
        p_.grad = None
    _, loss_dict0, _ = pipe.train_forward_backward(3)
    assert set(loss_dict0) == {"main_loss"}                       # exactly the keys without the feature
    depth_part = (total - model.means.grad).cpu().numpy()
    # oracle: 0.5 * mean over the valid pixels of |depth - stored depth| in float64
    Pp = {k: v.copy() for k, v in P.items()}
    Pp["means"] = (P["means"] + shift).astype(np.float32)
    assert np.array_equal(Pp["means"], model.means.detach().cpu().numpy())
    p = {k: torch.tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in Pp.items()}
    o = rt.get_outputs(p, torch.tensor(c2ws[VIEW]), K["fx"], K["fy"], K["cx"], K["cy"], W, H, torch.zeros(3), training=False, dtype=torch.float64)
    ref = dm.train_data[VIEW]["depth_image"].double().cpu()
    d = o["depth"][..., 0]
    valid = (d != 1000.0) & (ref != 1000.0)
    loss = 0.5 * (torch.where(valid, d - ref, torch.zeros_like(d)).abs().sum() / valid.sum().clamp(min=1))
    loss.backward()
    want = p["means"].grad.numpy()
    assert np.abs(want).max() > 0
    _grad_close(depth_part, want, float(np.abs(want).max()))
