"""The workbench without a GPU (vp_suite_amd.VPSuite, compatibility, the copy baseline): the run configuration against the reference's
table, the refusals, both compatibility checks on stub objects, and CopyLastFrame on host tensors."""
import importlib.util
import warnings

import pytest
import torch
from torch import nn

# DefaultRunConfig of the reference (vp_suite/defaults.py:37-64), key: default
REFERENCE_RUN_CONFIG = {
    "no_train": False, "no_val": False, "no_vis": False, "no_wandb": False, "vis_every": 10, "n_vis": 5, "vis_mode": "gif", "vis_compare": False,
    "vis_context_frame_idx": None, "seed": 42, "lr": 0.0001, "epochs": 1000000, "max_training_hours": 48, "batch_size": 32,
    "losses_and_scales": {"mse": 1.0}, "val_rec_criterion": "mse", "metrics": ["mse", "lpips", "psnr", "ssim"], "context_frames": 10,
    "pred_frames": 10, "seq_step": 1, "use_actions": False, "out_dir": None,
}


def test_default_run_config_is_the_references_with_the_stated_divergences(vpx):
    from vp_suite_amd.vpsuite import ADDED_RUN_KEYS, DEFAULT_RUN_CONFIG
    assert vpx.DEFAULT_RUN_CONFIG is DEFAULT_RUN_CONFIG
    want = dict(REFERENCE_RUN_CONFIG, no_vis=True, no_wandb=True, metrics=["mse", "psnr", "ssim"], test_batch_size=1, flat_adam=False)
    assert DEFAULT_RUN_CONFIG == want
    assert set(DEFAULT_RUN_CONFIG) - set(REFERENCE_RUN_CONFIG) == set(ADDED_RUN_KEYS) == {"test_batch_size", "flat_adam"}
    doc = vpx.vpsuite.__doc__
    for word in ("no_vis", "no_wandb", "lpips", "test_batch_size", "flat_adam", "DataLoader", "download_dataset"):
        assert word in doc, word


@pytest.fixture
def suite(vpx):
    """A suite on the host with the copy baseline and a tiny generated training set: enough for every check made before a launch."""
    s = vpx.VPSuite(device="cpu")
    s.load_dataset("MMF", digits=vpx.datasets.procedural_digits(n=4, size=8), n_seqs=2, img_size=16, num_channels=1)
    s.create_model("copy")
    return s


def test_run_kwargs_are_checked_and_seeds_are_set(vpx, suite):
    with pytest.raises(ValueError, match="Only the following run arguments are supported"):
        suite.train(learning_rate=0.1)
    with pytest.raises(ValueError, match="Only the following run arguments are supported"):
        suite._prepare_run("train", num_workers=4)
    with pytest.raises(NotImplementedError, match="no_vis"):
        suite.train(no_vis=False)
    with pytest.raises(NotImplementedError, match="no_wandb"):
        suite.train(no_wandb=False)
    with pytest.raises(ValueError, match="No test sets loaded"):
        suite.test()
    cfg = suite._prepare_run("train", seed=7, val_rec_criterion="psnr")
    assert cfg["opt_direction"] == "maximize" and cfg["seed"] == 7 and vpx.DEFAULT_RUN_CONFIG["seed"] == 42
    a = (torch.rand(1).item(), __import__("random").random(), __import__("numpy").random.rand())
    suite._prepare_run("train", seed=7)
    assert a == (torch.rand(1).item(), __import__("random").random(), __import__("numpy").random.rand())
    assert suite._prepare_run("train")["opt_direction"] == "minimize"
    with pytest.raises(RuntimeError, match="No model available"):
        vpx.VPSuite(device="cpu").train()


def test_suite_surface(vpx, suite, capsys):
    assert len(suite.training_sets) == 1 and suite.test_sets == [] and suite.datasets[0].NAME == "Moving MNIST - On the fly"
    wrapper = suite.datasets[0]
    assert not wrapper.is_ready and wrapper.train_data is not wrapper.val_data and wrapper.val_data.split == "val"
    with pytest.raises(KeyError):
        wrapper.test_data
    wrapper.set_seq_len(3, 2, 1)
    assert wrapper.is_ready and wrapper.val_data.ready_for_usage and wrapper.config["img_shape"] == (1, 16, 16)
    with pytest.raises(NotImplementedError, match="downloaded"):
        suite.download_dataset("MMF")
    with pytest.raises(ValueError, match="invalid model type"):
        suite.create_model("lstm")
    capsys.readouterr()
    suite.list_available_models()
    suite.list_available_datasets()
    said = capsys.readouterr().out
    assert "'copy': CopyLastFrame" in said and "'convlstm-shi'" in said and "'MMF': Moving MNIST - On the fly" in said
    # required arguments come from the last loaded dataset
    suite.create_model("unet-3d", temporal_dim=3)
    m = suite.models[-1]
    assert m.img_shape == (1, 16, 16) and m.action_size == 0 and list(m.tensor_value_range) == [0.0, 1.0] and m.action_conditional is False
    with pytest.raises(ValueError, match="no dataset loaded"):
        vpx.VPSuite(device="cpu").create_model("unet-3d")
    suite.clear_models()
    suite.clear_datasets()
    assert suite.models == [] and suite.datasets == []
    with pytest.raises(ValueError, match="needs to be one of"):
        suite.load_dataset("MMF", split="val", digits=vpx.datasets.procedural_digits(n=4, size=8))


@pytest.mark.skipif(importlib.util.find_spec("optuna") is not None, reason="optuna is installed: the ImportError cannot be seen")
def test_hyperopt_needs_optuna(suite):
    with pytest.raises(ImportError, match="optuna"):
        suite.hyperopt({"lr": {"type": "float", "min": 1e-5, "max": 1e-3, "scale": "log"}}, n_trials=1)


# ---- compatibility checks on stubs ------------------------------------------------------------------------------------------------
class _Model:
    NAME, model_dir = "stub model", None

    def __init__(self, img_shape=(3, 64, 64), rng=(0.0, 1.0), can=False, ac=False, action_size=0, min_context=1):
        self.CAN_HANDLE_ACTIONS, self.MIN_CONTEXT_FRAMES = can, min_context
        self.config = {"img_shape": img_shape, "tensor_value_range": list(rng), "action_conditional": ac, "action_size": action_size}


class _Data:
    NAME = "stub data"

    def __init__(self, img_shape=(3, 64, 64), rng=(0.0, 1.0), **extra):
        self.config = {"img_shape": img_shape, "tensor_value_range": list(rng), "action_size": 0, **extra}


def test_model_and_data_compat(vpx):
    from vp_suite_amd.compatibility import FrameAdapter, check_model_and_data_compat as check
    for strict in (False, True):
        pre, post = check(_Model(), _Data(), strict_mode=strict)
        assert type(pre) is nn.Identity and type(post) is nn.Identity
    # value range only, size only, both: ONE adapter per direction, scale and resize fused
    for model, data, pre_want, post_want in [
        (_Model(rng=(-1.0, 1.0)), _Data(), ((0.0, 1.0), (-1.0, 1.0), None), ((-1.0, 1.0), (0.0, 1.0), None)),
        (_Model(img_shape=(3, 32, 48)), _Data(), ((0.0, 1.0), (0.0, 1.0), (32, 48)), ((0.0, 1.0), (0.0, 1.0), (64, 64))),
        (_Model(img_shape=(3, 128, 128), rng=(-1.0, 1.0)), _Data(rng=(0.0, 255.0)), ((0.0, 255.0), (-1.0, 1.0), (128, 128)), ((-1.0, 1.0), (0.0, 255.0), (64, 64))),
    ]:
        pre, post = check(model, data)
        assert type(pre) is FrameAdapter and type(post) is FrameAdapter and not list(pre.children())
        assert (pre.src_range, pre.dst_range, pre.out_hw) == pre_want and (post.src_range, post.dst_range, post.out_hw) == post_want
        with pytest.raises(ValueError, match="differ"):
            check(model, data, strict_mode=True)
    with pytest.raises(vpx.VpxError, match="GPU tensor"):   # the adapter is the HIP op: no quiet host path
        check(_Model(rng=(-1.0, 1.0)), _Data())[0](torch.zeros(1, 2, 3, 64, 64))
    for strict in (False, True):
        with pytest.raises(ValueError, match="1-channel images .* expects 3 channels"):
            check(_Model(), _Data(img_shape=(1, 64, 64)), strict_mode=strict)
    # action rules: only for a model that can handle actions AND is action-conditional
    with pytest.raises(ValueError, match="doesn't provide actions"):
        check(_Model(can=True, ac=True, action_size=2), _Data(supports_actions=False))
    with pytest.raises(ValueError, match="doesn't provide actions"):
        check(_Model(can=True, ac=True, action_size=2), _Data())
    with pytest.raises(ValueError, match="Action size"):
        check(_Model(can=True, ac=True, action_size=2), _Data(supports_actions=True, action_size=4))
    data = _Data(supports_actions=True)
    data.config["action_size"] = 2
    assert type(check(_Model(can=True, ac=True, action_size=2), data)[0]) is nn.Identity
    assert type(check(_Model(can=True, ac=False, action_size=2), _Data())[0]) is nn.Identity
    assert type(check(_Model(can=False, ac=True, action_size=2), _Data())[0]) is nn.Identity


def test_run_and_model_compat(vpx):
    from vp_suite_amd.compatibility import check_run_and_model_compat as check
    run = {"use_actions": False, "context_frames": 3}
    acts = {"use_actions": True, "context_frames": 3}
    with pytest.raises(ValueError, match="can't be invoked without using actions"):
        check(_Model(can=True, ac=True), run)
    check(_Model(can=True, ac=True), acts)
    with pytest.raises(ValueError, match="was trained without using actions"):
        check(_Model(can=True, ac=False), acts)
    check(_Model(can=True, ac=False), run)
    with pytest.warns(UserWarning, match="can't handle actions"):
        check(_Model(can=False), acts)
    # MIN_CONTEXT_FRAMES: the last branch of the chain — only for models that cannot handle actions, in a run without actions
    with pytest.raises(ValueError, match="needs at least 5 context frames"):
        check(_Model(can=False, min_context=5), run)
    check(_Model(can=False, min_context=3), run)
    check(_Model(can=True, min_context=5), run)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        check(_Model(can=False, min_context=5), acts)
    assert "elif" in check.__doc__ and "MIN_CONTEXT_FRAMES" in check.__doc__


def test_copy_last_frame_on_host_tensors(vpx):
    from vp_suite_amd.base import VPModel
    from vp_suite_amd.models import AVAILABLE_MODELS, MODEL_CLASSES
    from vp_suite_amd.models.copy_last_frame import CopyLastFrame
    assert "copy" in AVAILABLE_MODELS and MODEL_CLASSES["copy"] is CopyLastFrame
    assert (CopyLastFrame.NAME, CopyLastFrame.REQUIRED_ARGS, CopyLastFrame.TRAINABLE, CopyLastFrame.CAN_HANDLE_ACTIONS) == ("CopyLastFrame", [], False, False)
    m = CopyLastFrame()
    assert m.device is None and list(m.parameters()) == []
    cfg = m.config
    assert (cfg["img_h"], cfg["img_w"], cfg["img_c"], cfg["NAME"], cfg["action_conditional"]) == (None, None, None, "CopyLastFrame", False)
    x = torch.rand(2, 4, 3, 5, 6)
    assert torch.equal(m.pred_1(x), x[:, -1])
    pred, losses = m(x, pred_frames=3)
    assert losses is None and pred.shape == (2, 3, 3, 5, 6) and all(torch.equal(pred[:, t], x[:, -1]) for t in range(3))
    loop, _ = VPModel.forward(m, x, pred_frames=3)   # the base class's pred_1 loop
    assert torch.equal(pred, loop)
    full = MODEL_CLASSES["copy"]("cpu", action_size=3, img_shape=(3, 64, 64), temporal_dim=3, action_conditional=False, tensor_value_range=[0.0, 1.0])
    assert (full.config["img_h"], full.config["img_w"], full.config["img_c"]) == (64, 64, 3)
    inp, target, _ = m.unpack_data({"frames": x, "actions": torch.zeros(2, 4, 1)}, {"device": "cpu", "context_frames": 3, "pred_frames": 1})
    assert torch.equal(m(inp, pred_frames=1)[0][:, 0], x[:, 2]) and torch.equal(target, x[:, 3:])
