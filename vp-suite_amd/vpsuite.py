"""VPSuite: the workbench of the reference (vp_suite/vpsuite.py) restated on this package's own pieces — load datasets, create or load
models, train one model on one dataset, test every loaded model on every loaded test set.

    suite = VPSuite()
    suite.load_dataset("MMF", digits=procedural_digits())          # or "MM" with data_dir=...
    suite.create_model("convlstm-shi")
    suite.train(epochs=10)
    suite.load_dataset("MMF", split="test", digits=procedural_digits())
    results = suite.test()
    suite.visualize("vis_out", vis_idx=[0, 1, 2], vis_context_frame_idx=[0, 9])

DEFAULT_RUN_CONFIG is the reference's DefaultRunConfig (defaults.py:37-64) key for key. WHAT DIFFERS FROM THE REFERENCE, all of it here:
  * no_vis = True and no_wandb = True by default, and setting either to False raises NotImplementedError: train() and test() render
    nothing and log nothing to wandb. The vis_* / n_vis keys are kept so that a reference configuration is accepted.
  * Visualizations are made on request instead: suite.visualize(out_dir, vis_idx, ...) writes, for every loaded test set, what the
    reference's test() writes under no_vis=False — visualization.visualize_sequences over the models test() would evaluate: a bordered
    ground truth / prediction GIF per datapoint and model, a comparison PNG per datapoint, vis_info.txt. Each output is one canvas
    composed by one HIP launch (ops.vis_compose, csrc/vis.hip). GIFs carry no matplotlib titles, one-channel frames are shown as grey
    RGB, and there is no mp4 (visualization.py lists the departures).
  * metrics = ["mse", "psnr", "ssim"]: "lpips" needs pretrained weights this build does not ship, so it is not a default. After
    measure.register_lpips_weights(...) (AlexNet weights the user brings; nothing is downloaded) the reference's own list,
    metrics=["mse", "lpips", "psnr", "ssim"], runs in train() and test(); on one-channel data it fails with the measure's ValueError.
    "fvd" likewise joins a metrics list after measure.register_fvd_weights(...) (an I3D network the user brings); it has a value from 9
    predicted frames on and is dropped with a warning for frames whose channel count the registered stem does not take.
  * One added key, test_batch_size = 1: test() may evaluate several datapoints per launch. Per-horizon means stay means over
    DATAPOINTS (batch means weighted by batch size), so a ragged last batch changes nothing.
  * One added key, flat_adam = False: True trains with train.FlatAdam (one HIP kernel over flat buckets) instead of torch.optim.Adam.
    FlatAdam's gradient clipping (max_grad_norm, clip_grad_value, skip_nonfinite) has NO run-config key: train() builds the optimizer
    without it; a loop that wants it calls model.train_iter with its own FlatAdam.
  * Batches come from the datasets' own loader() — GPU batches made in this process. There are no DataLoader worker processes (the
    reference's num_workers=4 would open the card from four more processes).
  * A dataset that is generated on the fly has its generators reset before every validation pass and before every test pass, so that
    "the validation set" and "the test set" are the same sequences each time (the reference draws new ones on every pass, which makes
    the best-model comparison and repeated tests incomparable).
  * test() RETURNS its results, {dataset NAME: {model NAME: [metric dict per prediction horizon]}}, besides printing what the reference
    prints. Tested models that share a NAME are told apart by " #k", k = the position in the test set's list of models.
  * download_dataset() raises NotImplementedError: nothing is ever fetched.
  * Models bridge a differing value range / frame size through ONE fused HIP launch per direction (compatibility.FrameAdapter).
  * Actions. A stored dataset that carries actions ("BAIR", or StoredVPDataset(actions=...)) sets supports_actions = True in its
    `config`; no dataset of the reference sets the key its compatibility check reads, so there no dataset accepts an action-conditional
    model. When a run leaves `use_actions` open (it is not among the run arguments), it is taken as True for an action-conditional model
    whose dataset carries actions, so that load_dataset("BAIR") / create_model(..., action_conditional=True) / train() / test() runs as
    it stands; a given `use_actions` always holds, and with datasets without actions nothing changes. test() hands the batch's actions
    to every action-conditional model (the reference asks for a `use_actions` attribute that nothing ever sets, so its test() passes
    actions to no model)."""
import json
import os
import random
import time
import warnings
from copy import deepcopy
from datetime import datetime
from pathlib import Path

import numpy as np
import torch
from torch import nn

from .compatibility import check_model_and_data_compat, check_run_and_model_compat
from .dataset_wrapper import VPDatasetWrapper
from .datasets import DATASET_CLASSES
from .measure import LOSS_CLASSES, PredictionLossProvider, PredictionMetricProvider
from .models import AVAILABLE_MODELS, MODEL_CLASSES
from .models.copy_last_frame import CopyLastFrame
from .visualization import visualize_sequences

OUT_PATH = Path("vp_suite_out")   #: trained models go to a timestamped directory below it unless `out_dir` is given

DEFAULT_RUN_CONFIG = {
    "no_train": False,              # the training loop is skipped
    "no_val": False,                # the validation loop is skipped; the model is saved as the 'best' one after every epoch
    "no_vis": True,                 # (reference: False) — False raises NotImplementedError
    "no_wandb": True,               # (reference: False) — False raises NotImplementedError
    "vis_every": 10,
    "n_vis": 5,
    "vis_mode": "gif",
    "vis_compare": False,
    "vis_context_frame_idx": None,
    "seed": 42,                     # python, numpy and torch generators
    "lr": 0.0001,
    "epochs": 1000000,              # large: by default a run ends by its time limit
    "max_training_hours": 48,       # the epoch that exceeds it is finished and becomes the last one
    "batch_size": 32,
    "losses_and_scales": {"mse": 1.0},
    "val_rec_criterion": "mse",
    "metrics": ["mse", "psnr", "ssim"],   # (reference: + "lpips")
    "context_frames": 10,
    "pred_frames": 10,
    "seq_step": 1,
    "use_actions": False,
    "out_dir": None,
    "test_batch_size": 1,           # (added) datapoints per test batch
    "flat_adam": False,             # (added) train with train.FlatAdam
}
ADDED_RUN_KEYS = ("test_batch_size", "flat_adam")


def timestamp(program: str):
    return f"{program}_{str(datetime.now()).split('.')[0].replace(' ', '_').replace(':', '-')}"


def check_optuna_config(optuna_cfg: dict):
    """Prints a notice when the optuna configuration is malformed (utils/utils.py:88-110)."""
    try:
        for p_dict in optuna_cfg.values():
            if not isinstance(p_dict, dict):
                raise ValueError
            if "choices" in p_dict:
                if not isinstance(p_dict["choices"], list):
                    raise ValueError
            else:
                if not {"type", "min", "max"}.issubset(p_dict) or p_dict["min"] > p_dict["max"]:
                    raise ValueError
                if p_dict["type"] == "float" and p_dict.get("scale", "") not in ["log", "uniform"]:
                    raise ValueError
    except ValueError:
        print("invalid optuna config")


def _loader(data, batch_size, shuffle, drop_last, seed=None):
    return data.loader(batch_size, shuffle=shuffle, drop_last=drop_last, seed=seed)


class VPSuite:
    """The workbench: `datasets` (VPDatasetWrapper) and `models` (VPModel) are the loaded ones, the last in each list the latest."""

    def __init__(self, device: str = "cuda"):
        self.device = "cuda" if device == "cuda" and torch.cuda.is_available() else "cpu"
        self.clear_models()
        self.clear_datasets()

    @property
    def training_sets(self):
        return [d for d in self.datasets if d.is_training_set()]

    @property
    def test_sets(self):
        return [d for d in self.datasets if d.is_test_set()]

    def clear_datasets(self):
        self.datasets = []

    def clear_models(self):
        self.models = []

    def load_dataset(self, dataset_id: str, split: str = "train", **dataset_kwargs):
        """Creates the dataset registered under dataset_id (training / validation data for split "train", test data for "test")."""
        dataset_class = DATASET_CLASSES[dataset_id]
        dataset = VPDatasetWrapper(dataset_class, split, **dataset_kwargs)
        print(f"loaded dataset '{dataset.NAME}' from {dataset.data_dir} (action size: {dataset.action_size})")
        if any(k in dataset_kwargs for k in ["context_frames", "pred_frames", "seq_step"]):
            dataset.set_seq_len(dataset_kwargs.pop("context_frames", DEFAULT_RUN_CONFIG["context_frames"]),
                                dataset_kwargs.pop("pred_frames", DEFAULT_RUN_CONFIG["pred_frames"]),
                                dataset_kwargs.pop("seq_step", DEFAULT_RUN_CONFIG["seq_step"]))
        self.datasets.append(dataset)

    def download_dataset(self, dataset_id: str):
        raise NotImplementedError("nothing is ever downloaded by this build: bring the files and pass data_dir= (or a glyph table, digits=)")

    def list_available_datasets(self):
        for dataset_id, dataset_class in DATASET_CLASSES.items():
            print(f"'{dataset_id}': {dataset_class.NAME}")

    def list_available_models(self):
        for model_id, model_class in MODEL_CLASSES.items():
            print(f"'{model_id}': {model_class.NAME}")

    def load_model(self, model_dir: str, ckpt_name: str = "best_model.pth"):
        """Loads the whole-module pickle train() saved (trusted files only, as with every pickle)."""
        model = torch.load(os.path.join(model_dir, ckpt_name), map_location=self.device, weights_only=False)
        model.model_dir = model_dir
        self._model_setup(model, loaded=True)

    def create_model(self, model_id: str, action_conditional: bool = False, **model_kwargs):
        """Creates the model registered under model_id; required arguments that are not given come from the last loaded dataset."""
        if model_id not in AVAILABLE_MODELS:
            raise ValueError(f"invalid model type specified! Available model types: {list(AVAILABLE_MODELS)}")
        model_class = MODEL_CLASSES[model_id]
        for param in model_class.REQUIRED_ARGS:
            if param not in model_kwargs:
                print(f"model parameter '{param}' not specified -> trying to take from last loaded dataset...")
                if len(self.datasets) < 1:
                    raise ValueError(f"no dataset loaded to take parameter '{param}' from")
                param_val = self.datasets[-1].config.get(param, None)
                if param_val is None:
                    raise ValueError(f"dataset '{self.datasets[-1].NAME}' doesn't provide parameter '{param}', "
                                     f"so it has to be specified on model creation")
                model_kwargs.update({param: param_val})
        if action_conditional and not model_class.CAN_HANDLE_ACTIONS:
            warnings.warn("specified model can't handle actions -> argument 'action_conditional' set to False")
            action_conditional = False
        model_kwargs.update(action_conditional=action_conditional)
        model = model_class(self.device, **model_kwargs).to(self.device)
        self._model_setup(model)

    def _model_setup(self, model, loaded: bool = False):
        ac_str = "(action-conditional)" if model.config["action_conditional"] else ""
        print(f"{'loaded' if loaded else 'created new'} model '{model.NAME}' {ac_str}")
        total_params = sum(p.numel() for p in model.parameters())
        trainable_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
        print(f" - Model parameters (total / trainable): {total_params} / {trainable_params}")
        self.models.append(model)

    def _prepare_run(self, split: str = "train", **run_kwargs):
        if len(self.models) == 0:
            raise RuntimeError("No model available. Load a pretrained model "
                               "or create a new instance before starting training or test runs")
        if split == "train" and len(self.training_sets) == 0:
            raise ValueError("No training sets loaded. Load a dataset in training mode "
                             "before starting training or test runs")
        elif split == "test" and len(self.test_sets) == 0:
            raise ValueError("No test sets loaded. Load a dataset in test mode "
                             "before starting training or test runs")
        run_config = deepcopy(DEFAULT_RUN_CONFIG)
        if not all(run_arg in run_config for run_arg in run_kwargs):
            raise ValueError(f"Only the following run arguments are supported: {list(run_config.keys())}")
        run_config.update(run_kwargs)
        if not run_config["no_vis"]:
            raise NotImplementedError("no_vis=False: rendering visualizations (gif / mp4) is not part of this build")
        if not run_config["no_wandb"]:
            raise NotImplementedError("no_wandb=False: logging to Weights and Biases is not part of this build")
        self._set_seeds(run_config["seed"])
        run_config["opt_direction"] = "maximize" if LOSS_CLASSES[run_config["val_rec_criterion"]].BIGGER_IS_BETTER else "minimize"
        return run_config

    @staticmethod
    def _open_use_actions(run_config: dict, run_kwargs: dict, model, datasets):
        """`run_config`, or a copy with use_actions = True when the caller left the key open, `model` is action-conditional and one of
        `datasets` carries actions (see the module docstring)."""
        if "use_actions" in run_kwargs or not (model.CAN_HANDLE_ACTIONS and model.config["action_conditional"]):
            return run_config
        if not any(d.config.get("supports_actions", False) for d in datasets):
            return run_config
        return {**run_config, "use_actions": True}

    def _set_seeds(self, seed: int):
        """The only place where the general generators are seeded."""
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)

    def reset_rng(self, seed: int):
        self._set_seeds(seed)
        for dataset in self.datasets:
            dataset.reset_rng()

    # ===== TRAINING ================================================================

    def _prepare_training(self, dataset_idx: int, model_idx: int, **run_kwargs):
        run_config = self._prepare_run("train", **run_kwargs)
        try:
            dataset = self.training_sets[dataset_idx]
            model = self.models[model_idx]
        except IndexError:
            raise ValueError("given indices for model and/or dataset are invalid")
        dataset.set_seq_len(run_config["context_frames"], run_config["pred_frames"], run_config["seq_step"])
        assert dataset.is_ready, "dataset is not ready even though set_seq_len has just been called"
        run_config = self._open_use_actions(run_config, run_kwargs, model, [dataset])
        check_run_and_model_compat(model, run_config)
        check_model_and_data_compat(model, dataset, strict_mode=True)
        return model, dataset, run_config

    def train(self, trial=None, dataset_idx: int = -1, model_idx: int = -1, **run_kwargs):
        """Trains one model on one training set until `epochs` or `max_training_hours` is reached: per epoch one model.train_iter over
        the training data, then one model.eval_iter over the validation data at batch size 1; the model is saved as best_model.pth
        whenever the validation criterion improved (after every epoch under no_val), and as final_model.pth at the end, next to
        run_cfg.json. Returns the best validation loss."""
        model, dataset, run_config = self._prepare_training(dataset_idx, model_idx, **run_kwargs)
        train_data, val_data = dataset.train_data, dataset.val_data
        train_loader = _loader(train_data, run_config["batch_size"], shuffle=True, drop_last=True, seed=run_config["seed"])
        val_loader = _loader(val_data, 1, shuffle=False, drop_last=True)
        best_val_loss = float("inf")

        # re-use model_dir of pre-loaded/pre-initialized models if no out_dir has been specified
        if run_config["out_dir"] is None and model.model_dir is not None:
            print(f"Using existing model save location ({model.model_dir})...")
            out_path = Path(model.model_dir)
        else:
            out_path = Path(run_config["out_dir"] or OUT_PATH / timestamp("train"))
            out_path.mkdir(parents=True, exist_ok=True)
            model.model_dir = str(out_path.resolve())
        best_model_path = str((out_path / "best_model.pth").resolve())
        with_training = model.TRAINABLE and not run_config["no_train"]
        with_validation = not run_config["no_val"]

        # hyperparameter optimization
        optuna_config = run_config.get("optuna", None)
        if trial is not None and isinstance(optuna_config, dict):
            for param, p_dict in optuna_config.items():
                if "choices" in p_dict:
                    if param == "model_type":
                        warnings.warn(f"hyperopt across model and dataset parameters is not yet supported -> using {model.NAME}")
                    run_config[param] = trial.suggest_categorical(param, p_dict["choices"])
                else:
                    suggest = trial.suggest_int if p_dict["type"] == "int" else trial.suggest_float
                    if p_dict.get("scale", "uniform") == "log":
                        run_config[param] = suggest(param, p_dict["min"], p_dict["max"], log=True)
                    else:
                        run_config[param] = suggest(param, p_dict["min"], p_dict["max"], step=p_dict.get("step", 1))

        # assemble and save combined configuration
        config = {**run_config, **model.config, **dataset.config, "device": self.device,
                  "model_name": model.NAME, "dataset_name": dataset.NAME}
        save_config = {"run": run_config, "model": model.config, "dataset": dataset.config, "device": self.device}
        with open(str((out_path / "run_cfg.json").resolve()), "w") as cfg_file:
            json.dump(save_config, cfg_file, indent=4, default=lambda o: str(o))

        # optimizer
        optimizer, optimizer_scheduler = None, None
        if with_training:
            if run_config["flat_adam"]:
                from .train import FlatAdam
                optimizer = FlatAdam.from_module(model, lr=run_config["lr"])
            else:
                optimizer = torch.optim.Adam(params=model.parameters(), lr=run_config["lr"])
            optimizer_scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=5, factor=0.2, min_lr=1e-6)

        # losses and measurement
        loss_provider = PredictionLossProvider(config)
        if config["val_rec_criterion"] not in config["losses_and_scales"]:
            raise ValueError(f"Validation criterion '{config['val_rec_criterion']}' has to be "
                             f"one of the chosen losses: {list(config['losses_and_scales'].keys())}")
        if config["opt_direction"] == "maximize":
            def loss_improved(cur_loss, best_loss): return cur_loss > best_loss
        else:
            def loss_improved(cur_loss, best_loss): return cur_loss < best_loss

        # --- main loop ---
        training_timeout = time.time() + config["max_training_hours"] * 3600
        for epoch in range(0, run_config["epochs"]):
            print(f"\nEpoch: {epoch + 1} of {config['epochs']}")
            if with_training:
                print("Training...")
                model.train_iter(config, train_loader, optimizer, loss_provider, epoch)
            else:
                print("Skipping training loop.")

            if with_validation:
                print("Validating...")
                if getattr(val_data, "ON_THE_FLY", False):
                    val_data.reset_rng()   # the same validation sequences in every epoch
                val_losses, indicator_loss = model.eval_iter(config, val_loader, loss_provider)
                if with_training:
                    optimizer_scheduler.step(indicator_loss)
                print("Validation losses (mean over entire validation set):")
                for k, v in val_losses.items():
                    print(f" - {k}: {v}")
                cur_val_loss = indicator_loss.item()
                if loss_improved(cur_val_loss, best_val_loss):
                    best_val_loss = cur_val_loss
                    torch.save(model, best_model_path)
                    print(f"Minimum indicator loss ({config['val_rec_criterion']}) reduced -> model saved!")
            else:
                print("Skipping validation loop and simply saving current model as the 'best' model.")
                torch.save(model, best_model_path)

            if time.time() > training_timeout:
                print("Maximum training time exceeded, leaving training loop...")
                break

        print("\nTraining done, cleaning up...")
        torch.save(model, str((out_path / "final_model.pth").resolve()))
        return best_val_loss  # (the objective of a hyperparameter optimization)

    def hyperopt(self, optuna_config: dict, n_trials: int = 30, dataset_idx: int = -1, model_idx: int = -1, **run_kwargs):
        """Hyperparameter optimization with optuna: n_trials training runs over the search space of optuna_config. optuna itself is not
        part of this build: without it this raises the reference's ImportError."""
        from functools import partial
        run_config = self._prepare_run(**run_kwargs)
        check_optuna_config(optuna_config)
        run_config["optuna"] = optuna_config
        try:
            import optuna
        except ImportError:
            raise ImportError("Importing optuna failed -> install it or use the code without the 'use-optuna' flag.")
        optuna_program = partial(self.train, dataset_idx=dataset_idx, model_idx=model_idx, **run_kwargs)
        study = optuna.create_study(direction=run_config["opt_direction"])
        study.optimize(optuna_program, n_trials=n_trials)
        print("\nHyperparameter optimization complete. Best performing parameters:")
        for k, v in study.best_params.items():
            print(f" - {k}: {v}")

    # ===== TESTING ================================================================

    def _prepare_testing(self, **run_kwargs):
        """Sets the test sets' sequence length and lists, per test set, the models that pass the compatibility checks (with their
        adapters) plus the copy baseline. Incompatible models are skipped with a message."""
        run_config = self._prepare_run("test", **run_kwargs)
        test_sets = self.test_sets
        for test_set in test_sets:
            test_set.set_seq_len(run_config["context_frames"], run_config["pred_frames"], run_config["seq_step"])
            assert test_set.is_ready, "test set is not ready even though set_seq_len has just been called"

        test_models = []
        for model in self.models:
            try:
                check_run_and_model_compat(model, self._open_use_actions(run_config, run_kwargs, model, test_sets))
                test_models.append(model)
            except ValueError as e:
                print(f"skipping test of model '{model.NAME}' because of incompatibility with run config: {str(e)}")

        model_lists_all_test_sets = []
        for test_set in test_sets:
            test_set_model_list = []
            for model in test_models:
                try:
                    preprocessing, postprocessing = check_model_and_data_compat(model, test_set)
                    test_set_model_list.append((model, preprocessing, postprocessing, []))
                except ValueError as e:
                    print(f"skipping test of model '{model.NAME}' on dataset '{test_set.NAME}' "
                          f"because of incompatibility: {str(e)}")
            model_lists_all_test_sets.append(test_set_model_list)
            # add baseline copy model (doesn't need checks)
            clf_baseline = CopyLastFrame().to(self.device)
            test_set_model_list.append((clf_baseline, nn.Identity(), nn.Identity(), []))
        return zip(test_sets, model_lists_all_test_sets), run_config

    def _test_on_dataset(self, model_info_list, dataset, run_config: dict, brief_test: bool):
        """Every listed model on every datapoint of one test set (10 at the most if brief_test). Returns {model NAME: [metric dict per
        prediction horizon]}: means over the datapoints."""
        test_data = dataset.test_data
        if len(test_data) < 1:
            raise RuntimeError("loaded dataset does not contain any data (len < 1)")
        if getattr(test_data, "ON_THE_FLY", False):
            test_data.reset_rng()   # the same test sequences in every test run
        test_loader = _loader(test_data, run_config["test_batch_size"], shuffle=False, drop_last=False)
        test_mode = "brief" if brief_test else "full"
        eval_length = min(len(test_data), 10) if brief_test else len(test_data)   # datapoints

        config = {**run_config, **dataset.config, "device": self.device, "dataset_name": dataset.NAME}
        pred_frames = config["pred_frames"]
        seen = 0
        with torch.no_grad():
            metric_provider = PredictionMetricProvider(config)
            for data in test_loader:
                if seen >= eval_length:
                    break
                n = int(data["frames"].shape[0])
                if seen + n > eval_length:   # the brief test ends inside this batch
                    n = eval_length - seen
                    data = {**data, "frames": data["frames"][:n], "actions": data["actions"][:n]}
                seen += n
                for (model, preprocess, postprocess, model_metrics_per_batch) in model_info_list:
                    inp, target, actions = model.unpack_data(data, config)
                    inp = preprocess(inp)  # test format to model format
                    model.eval()
                    if model.CAN_HANDLE_ACTIONS and model.config["action_conditional"]:   # (the reference: an attribute nothing sets)
                        pred, _ = model(inp, pred_frames=pred_frames, actions=actions)
                    else:
                        pred, _ = model(inp, pred_frames=pred_frames)
                    model.train()
                    pred = postprocess(pred)  # model format to test format
                    cur_metrics = metric_provider.get_metrics(pred, target, all_frame_cnts=True)
                    model_metrics_per_batch.append((n, cur_metrics))

        results = {}
        for i, (model, _, _, model_metrics_per_batch) in enumerate(model_info_list):
            # model_metrics_per_batch: per batch (datapoints n, F metric dicts: the batch's means for a prediction horizon of f frames)
            # -> means over all datapoints, the metrics and prediction horizons kept apart
            total = sum(n for n, _ in model_metrics_per_batch)
            frame_range = range(len(model_metrics_per_batch[0][1]))
            # (the keys of each horizon's own dict: "fvd" has a value from 9 frames on only)
            mean_metric_dicts = [{key: float(sum(n * dicts[frame][key] for n, dicts in model_metrics_per_batch) / total)
                                  for key in model_metrics_per_batch[0][1][frame].keys()} for frame in frame_range]
            name = model.NAME if model.NAME not in results else f"{model.NAME} #{i}"
            results[name] = mean_metric_dicts
            print(f"\n{model.NAME} (path: {model.model_dir}, {test_mode} test): ")
            for f, mean_metric_dict in enumerate(mean_metric_dicts):
                print(f"pred_frames: {f + 1}")
                for (k, v) in mean_metric_dict.items():
                    print(f" -> {k}: {v}")
        return results

    def test(self, brief_test=False, **run_kwargs):
        """Tests all loaded models on all loaded test sets, one set after the other; returns {dataset NAME: {model NAME: [metric dict
        per prediction horizon]}}."""
        test_sets_and_model_lists, run_config = self._prepare_testing(**run_kwargs)
        results = {}
        for test_set, model_info_list in test_sets_and_model_lists:
            results[test_set.NAME] = self._test_on_dataset(model_info_list, test_set, run_config, brief_test)
        return results

    # ===== VISUALIZATION ================================================================

    def visualize(self, out_dir, vis_idx, vis_context_frame_idx=None, vis_vid_mode: str = "gif", **run_kwargs):
        """Saves prediction visualizations of the datapoints `vis_idx` of every loaded test set, for the models test() would evaluate on
        it (the same compatibility checks, the same frame adapters; models without a model_dir, such as the copy baseline, are left
        out): per datapoint i and model j the bordered side-by-side video vis_<i>_model_<j>.gif of ground truth and prediction, and — if
        vis_context_frame_idx is given — the comparison image vis_<i>.png of all models against the ground truth, plus vis_info.txt.
        With one test set the files go to out_dir, with several to out_dir/<k> for the k-th. run_kwargs as for test(). Returns the
        directories written, one per test set."""
        if vis_vid_mode != "gif":
            raise NotImplementedError(f"vis mode '{vis_vid_mode}': this build has no video encoder -> use the gif-mode for visualization")
        test_sets_and_model_lists, run_config = self._prepare_testing(**run_kwargs)
        test_sets_and_model_lists = list(test_sets_and_model_lists)
        written = []
        for k, (test_set, model_info_list) in enumerate(test_sets_and_model_lists):
            test_data = test_set.test_data
            out_path = Path(out_dir) if len(test_sets_and_model_lists) == 1 else Path(out_dir) / str(k)
            out_path.mkdir(parents=True, exist_ok=True)
            if getattr(test_data, "ON_THE_FLY", False):
                test_data.reset_rng()   # the same sequences in every run
            visualize_sequences(test_data, run_config["context_frames"], run_config["pred_frames"], model_info_list, self.device, out_path,
                                vis_idx, vis_context_frame_idx, vis_vid_mode)
            written.append(str(out_path))
        return written
