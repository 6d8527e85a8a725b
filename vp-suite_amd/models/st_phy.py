"""ST-Phy ("st-phy") — drop-in for vp_suite/models/st_phy.py: the reference's class constants, hyper-parameters, `state_dict` (83
entries, 6 772 922 parameters at 1x64x64) and `forward(x, pred_frames, train=, teacher_forcing=)` contract, on the library's kernels:
the autoencoder's convolutions with ReLU in their epilogue and the encoder tail (stphy_ops), the ST-LSTM step with LayerNorm, the
PhyCell, the two-source merge, the batched decoupling term and the fp64 moment loss. No ATen convolution, normalisation or
activation runs over activations.

What the reference computes, kept as it is (st_phy.py:126-181):
  * every layer's cells get the SAME `next_input`, and `x_gen` is overwritten per layer: only the last layer's merge and PhyCell
    reach an output; the lower ST cells stay live through `st_memory` and the decoupling term;
  * the moment loss reads `phycell_list[0].F.conv1.weight` (also when that cell is otherwise dead) and `moment_loss_scale` is applied
    twice (inside the mean and outside it);
  * under `train=True` every step decodes (context + pred - 1 frames) and both model losses exist; in eval the result has
    `pred_frames` frames and the second return value is None.

The step schedule differs from the reference's only in work nothing can observe (outputs are unchanged):
  * all frames known up front (the context frames; under teacher forcing every frame) are encoded in ONE batch;
  * all frames are decoded after the recurrence in one batch: an autoregressive step feeds the merged latent `x_gen` back, not the
    decoded frame (st_phy.py:132), so no step has to decode on the spot;
  * in eval the context steps are not decoded at all;
  * in eval the adapter / normalisation work of st_phy.py:148-149 is skipped (it only feeds the decoupling loss, which exists
    under `train=True` alone); in training the decoupling terms of the whole pass are one `ops.decouple_term_batched` call;
  * the PhyCells and merge convolutions of layers < num_layers - 1 are skipped: their results are overwritten before anything
    reads them. Their parameters therefore get no gradient (`.grad` stays None), as in the reference, where it is None too — except
    `phycell_list.0.F.conv1.weight`, which the moment loss reaches.

Divergences, stated loudly:
  * the action-conditional variant needs (5,1) and (1,5) convolutions, which the library's single-padding convolution cannot
    express: `CAN_HANDLE_ACTIONS = False`, and `action_conditional=True` raises NotImplementedError at construction;
  * frame sizes where the decoder's `Resize` is not the identity (anything but multiples of 4 from 20 up) raise ValueError at
    construction; `phycell_kernel_size` must be square and odd (PhyCell_Cell)."""
import random

import numpy as np
import torch
from torch import nn

from .. import ops, phy_ops, stphy_ops
from ..base import VPModel, _progress
from ..model_blocks.enc import Autoencoder
from ..model_blocks.phydnet import PhyCell_Cell
from ..model_blocks.predrnn import SpatioTemporalLSTMCell

PRECISIONS = ("f32", "bf16x3")


class STPhy(VPModel):
    NAME = "ST-Phy"
    CAN_HANDLE_ACTIONS = False   # (the reference: True — see the module docstring)

    num_layers = 3  #: Number of layers (1 PhyCell and 1 ST cell per layer)
    phycell_channels = 49  #: Channel dimensionality for the PhyCells
    phycell_kernel_size = (7, 7)  #: PhyCell kernel size
    st_cell_channels = 64  #: Hidden layer dimensionality for the ST cell layers
    inflated_action_dim = 3  #: Dimensionality of the 'inflated actions' (actions that have been transformed to tensors)

    decoupling_loss_scale = 100.0  #: The scaling factor for the decoupling loss
    moment_loss_scale = 1.0  #: Scaling factor for the moment loss (for PDE-Constrained prediction by the PhyCells)
    teacher_forcing_decay = 0.003  #: Per-Episode decrease of the teacher forcing ratio (Starts out at 1.0)
    cell_precision = "f32"  #: arithmetic of the convolutions and the cells ("f32" | "bf16x3")
    training_epoch = 0  #: epoch of the teacher-forcing schedule when training_loss draws it (train_iter sets it)

    def __init__(self, device, **model_kwargs):
        super().__init__(device, **model_kwargs)
        self.NON_CONFIG_VARS.append("training_epoch")
        if self.cell_precision not in PRECISIONS:
            raise ValueError(f"STPhy: cell_precision must be one of {PRECISIONS}, got {self.cell_precision!r}")
        if self.action_conditional:
            raise NotImplementedError("STPhy: the action-conditional variant needs (5,1) / (1,5) convolutions, which the library's "
                                      "single-padding convolution cannot express")
        if self.num_layers < 1:
            raise ValueError(f"STPhy: num_layers must be at least 1, got {self.num_layers}")
        self.dim_st_hidden = [self.st_cell_channels] * self.num_layers
        self.dim_phy_hidden = [self.phycell_channels] * self.num_layers

        self.autoencoder = Autoencoder(self.img_shape, self.st_cell_channels, self.device)   # (ValueError for unsupported frame sizes)
        _, _, self.enc_h, self.enc_w = self.autoencoder.encoded_shape

        st_cells, phycells, hidden_convs = [], [], []
        for i in range(self.num_layers):
            cell_in_channel = self.dim_st_hidden[0] if i == 0 else self.dim_st_hidden[i - 1]
            st_cells.append(SpatioTemporalLSTMCell(cell_in_channel, self.dim_st_hidden[i], self.enc_h, self.enc_w, filter_size=5, stride=1,
                                                   layer_norm=True))
            phycells.append(PhyCell_Cell(input_dim=cell_in_channel, action_conditional=False, action_size=self.action_size,
                                         hidden_dim=self.dim_phy_hidden[i], kernel_size=self.phycell_kernel_size).to(self.device))
            hidden_convs.append(nn.Conv2d(in_channels=self.st_cell_channels + self.dim_st_hidden[i], out_channels=self.st_cell_channels,
                                          kernel_size=(1, 1), bias=i < self.num_layers - 1))
        self.st_cell_list = nn.ModuleList(st_cells)
        self.phycell_list = nn.ModuleList(phycells)
        self.hidden_conv_list = nn.ModuleList(hidden_convs)
        self.adapter = nn.Conv2d(self.dim_st_hidden[0], self.dim_st_hidden[0], 1, stride=1, padding=0, bias=False)

        constraints = torch.zeros((self.phycell_channels, *self.phycell_kernel_size))
        ind = 0
        for i in range(0, self.phycell_kernel_size[0]):
            for j in range(0, self.phycell_kernel_size[1]):
                constraints[ind, i, j] = 1
                ind += 1
        # (what the moment-loss kernel builds on the fly; kept for the reference's attribute, out of the state_dict like there)
        self.register_buffer("constraints", constraints, persistent=False)
        for m in self.modules():
            if hasattr(type(m), "precision") and m is not self:
                m.precision = self.cell_precision
        self.to(self.device)

    def pred_1(self, x, **kwargs):
        return self(x, pred_frames=1, **kwargs)[0].squeeze(dim=1)

    # ---- the step schedule ---------------------------------------------------------------------------------------------------------
    def forward(self, x, pred_frames=1, **kwargs):
        train = kwargs.get("train", False)
        teacher_forcing = kwargs.get("teacher_forcing", False) and train
        b = x.shape[0]
        context_frames = x.shape[1] - pred_frames if train else x.shape[1]
        if context_frames < 1:
            raise ValueError(f"STPhy: {x.shape[1]} input frames leave no context frame for {pred_frames} predictions in training")
        if tuple(x.shape[2:]) != (self.img_c, self.img_h, self.img_w):
            raise ValueError(f"STPhy: frames of shape {tuple(x.shape[2:])}, the model was built for {(self.img_c, self.img_h, self.img_w)}")
        n_steps = context_frames + pred_frames - 1
        dev, prec, top, L = x.device, self.cell_precision, self.num_layers - 1, self.num_layers
        C, eh, ew = self.st_cell_channels, self.enc_h, self.enc_w

        # every frame whose encoder input is known before the recurrence starts, encoded in one batch (frame-major)
        n_known = min(n_steps, context_frames + (pred_frames - 1 if teacher_forcing else 0))
        known = x[:, :n_known].transpose(0, 1).reshape(n_known * b, *x.shape[2:])
        enc_all = self.autoencoder.encode(known)

        def zeros():
            return ops.new_channels_last((b, C, eh, ew), dev).zero_()
        st_h, st_c = [zeros() for _ in range(L)], [zeros() for _ in range(L)]
        st_memory, phy_h = zeros(), zeros()
        slab, deltas = None, []
        if train:   # [delta_c | delta_m][layer-step][sample]: the steps write their deltas into the slab the batched decoupling tail reads
            slab = ops.new_channels_last((2, n_steps * L * b, C, eh, ew), dev)

        first_out = 0 if train else context_frames - 1      # step whose output is result frame 0
        deferred = []                                       # merged maps of the steps that produce a frame, decoded after the loop
        hc = self.hidden_conv_list[top]
        x_gen = None
        for t in range(n_steps):
            next_input = enc_all[t * b:(t + 1) * b] if t < n_known else x_gen
            phy_h = self.phycell_list[top](next_input, None, phy_h)
            for i, cell in enumerate(self.st_cell_list):
                dout = None
                if slab is not None:
                    ls = t * L + i
                    dout = (slab[0, ls * b:(ls + 1) * b], slab[1, ls * b:(ls + 1) * b])
                st_h[i], st_c[i], st_memory, d_c, d_m = cell(next_input, st_h[i], st_c[i], st_memory, delta_out=dout, precision=prec)
                if slab is not None:
                    deltas += [d_c, d_m]
            x_gen = stphy_ops.merge1x1(st_h[top], phy_h, hc.weight, hc.bias, precision=prec)
            if t < first_out:
                continue
            deferred.append(x_gen)
        # (an autoregressive step consumes x_gen itself, not the decoded frame — st_phy.py:132 — so EVERY decode can wait)
        k = len(deferred)
        merged = torch.cat(deferred, dim=0) if k > 1 else deferred[0]
        frames = self.autoencoder.decode(merged)            # [k*b, c, H, W] frame-major
        out_frames = frames.reshape(k, b, *frames.shape[1:]).transpose(0, 1)

        if train:
            moment = phy_ops.moment_loss(self.phycell_list[0].F.conv1.weight, self.moment_loss_scale * self.moment_loss_scale)
            decoupling = ops.decouple_term_batched(slab, self.adapter.weight, prec, n_steps * L, b, deltas)
            model_losses = {"moment regularization loss": moment, "memory decoupling loss": self.decoupling_loss_scale * decoupling}
        else:
            model_losses = None
        return out_frames, model_losses

    # ---- training ------------------------------------------------------------------------------------------------------------------
    def _teacher_forcing_draw(self):
        """The reference's schedule (st_phy.py train_iter): teacher forcing with probability max(0, 1 - epoch * teacher_forcing_decay)."""
        return random.random() < np.maximum(0, 1 - self.training_epoch * self.teacher_forcing_decay)

    def training_loss(self, inp, targets, pred_frames, loss_provider, teacher_forcing=None, **fwd_kwargs):
        """Loss of ONE training iteration of the reference (st_phy.py train_iter), for train_iter and train.DataParallelTrainer alike.

        `inp` holds the context frames and `targets` the `pred_frames` frames that follow them (what `unpack_data` returns); the step runs
        the training forward over their concatenation and takes the image losses against every frame from the second one on, plus both
        model losses. `teacher_forcing=None` draws it from the schedule at `training_epoch`, which train_iter sets."""
        fwd_kwargs.pop("train", None)
        fwd_kwargs.pop("actions", None)   # (not action-conditional: the reference ignores them too)
        if targets is None or targets.dim() != inp.dim() or targets.shape[1] != pred_frames or targets.shape[0] != inp.shape[0]:
            raise ValueError(f"STPhy.training_loss: targets must hold the {pred_frames} frames that follow the context frames of `inp`, "
                             f"got {None if targets is None else tuple(targets.shape)} for input {tuple(inp.shape)}")
        if teacher_forcing is None:
            teacher_forcing = self._teacher_forcing_draw()
        full = torch.cat([inp, targets.to(inp.device)], dim=1)
        predictions, model_losses = self(full, pred_frames=pred_frames, train=True, teacher_forcing=teacher_forcing, **fwd_kwargs)
        return self._total_loss(predictions, full[:, 1:], model_losses, loss_provider)

    def train_iter(self, config, data_loader, optimizer, loss_provider, epoch):
        """One pass over `data_loader` with the reference's teacher-forcing schedule: per batch, teacher forcing with probability
        max(0, 1 - epoch * teacher_forcing_decay)."""
        self.training_epoch = epoch
        loop = _progress(data_loader)
        for data in loop:
            inp, targets, _ = self.unpack_data(data, config)
            total = self.training_loss(inp, targets, config["pred_frames"], loss_provider)
            optimizer.zero_grad()
            total.backward()
            optimizer.step()
            if hasattr(loop, "set_postfix"):
                loop.set_postfix(loss=total.item())
