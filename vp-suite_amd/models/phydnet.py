"""PhyDNet ("phy") — drop-in for vp_suite/models/phydnet.py: the reference's class constants, hyper-parameters, `state_dict` and
`forward(x, pred_frames, train=, teacher_forcing=, actions=)` contract, on the library's kernels (convolutions, GroupNorm + LeakyReLU,
the PhyCell correction, the fused ConvLSTM cell, the moment loss and the sigmoid head; no ATen convolution, normalisation or
activation runs over activations).

The step schedule differs from the reference's only in work nothing can observe (outputs are unchanged):
  * the two partial reconstructions `out_phys` / `out_conv` (two extra decoder passes per step, discarded by `forward`) are not computed;
  * the three encoders run ONCE, batched over every frame whose input is known up front (all context frames; under teacher forcing
    every frame); only the autoregressive prediction steps encode their own previous output one frame at a time;
  * under `train=False` the context steps are not decoded at all; in training their outputs (and, under teacher forcing, all outputs)
    are decoded batched after the recurrence;
  * `decoded_phys + decoded_conv` is added inside the GroupNorm kernel of the last `DecoderSplit` layer, and the sigmoid head writes
    each frame into its slot of the result (no torch.stack in inference).

Restrictions: frame height and width must be divisible by 4, where the reference's `Resize` is the identity (DCGANDecoder), and
`phycell_kernel_size` must be square and odd (PhyCell_Cell: the library's convolution takes one padding for both axes); both raise
ValueError at construction."""
import random

import numpy as np
import torch

from ..base import VPModel, _progress
from ..model_blocks.enc import DCGANDecoder, DCGANEncoder
from ..model_blocks.phydnet import DecoderSplit, EncoderSplit, PhyCell, SingleStepConvLSTM
from .. import phy_ops

PRECISIONS = ("f32", "bf16x3")


class PhyDNet(VPModel):
    NAME = "PhyDNet"
    PAPER_REFERENCE = "https://arxiv.org/abs/2003.01460"
    CODE_REFERENCE = "https://github.com/vincent-leguen/PhyDNet"
    MATCHES_REFERENCE: str = "Not Yet"
    CAN_HANDLE_ACTIONS = True

    phycell_n_layers = 1  #: Number of PhyCell layers
    phycell_channels = 49  #: Channel dimensionality for the PhyCells
    phycell_kernel_size = (7, 7)  #: PhyCell kernel size
    convlstm_n_layers = 3  #: Number of ConvCell layers
    convlstm_hidden_dims = [128, 128, 64]  #: Channel dimensionality per ConvCell layer
    convlstm_kernel_size = (3, 3)  #: ConvCell kernel size

    moment_loss_scale = 1.0  #: Scaling factor for the moment loss (for PDE-Constrained prediction by the PhyCells)
    teacher_forcing_decay = 0.003  #: Per-Episode decrease of the teacher forcing ratio (Starts out at 1.0)
    cell_precision = "f32"  #: arithmetic of the convolutions and the ConvLSTM cells ("f32" | "bf16x3")
    training_epoch = 0  #: epoch of the teacher-forcing schedule when training_loss draws it (train_iter sets it)

    def __init__(self, device, **model_kwargs):
        super().__init__(device, **model_kwargs)
        self.NON_CONFIG_VARS.append("training_epoch")
        if self.cell_precision not in PRECISIONS:
            raise ValueError(f"PhyDNet: cell_precision must be one of {PRECISIONS}, got {self.cell_precision!r}")
        if self.img_h % 4 or self.img_w % 4:
            raise ValueError(f"PhyDNet: frame size {self.img_h}x{self.img_w} is not divisible by 4 (the reference's Resize path for such "
                             f"sizes is not supported)")
        self.encoder_E = DCGANEncoder(img_channels=self.img_c).to(self.device)
        self.encoder_Ep = EncoderSplit().to(self.device)
        self.encoder_Er = EncoderSplit().to(self.device)
        # the reference runs the encoder on zeros for these: two stride-2 layers (k 3, pad 1) -> a quarter of the frame, 64 channels
        latent = torch.Size((64, self.img_h // 4, self.img_w // 4))
        self.shape_Ep, self.shape_Er = latent, latent

        self.decoder_Dp = DecoderSplit().to(self.device)
        self.decoder_Dr = DecoderSplit().to(self.device)
        self.decoder_D = DCGANDecoder(out_size=self.img_shape[1:], img_channels=self.img_c).to(self.device)

        phycell_hidden_dims = [self.phycell_channels] * self.phycell_n_layers
        self.phycell = PhyCell(input_size=self.shape_Ep[1:], input_dim=self.shape_Ep[0], hidden_dims=phycell_hidden_dims,
                               n_layers=self.phycell_n_layers, kernel_size=self.phycell_kernel_size,
                               action_conditional=self.action_conditional, action_size=self.action_size, device=device).to(self.device)
        self.convcell = SingleStepConvLSTM(input_size=self.shape_Er[1:], input_dim=self.shape_Ep[0], hidden_dims=self.convlstm_hidden_dims,
                                           n_layers=self.convlstm_n_layers, kernel_size=self.convlstm_kernel_size,
                                           action_conditional=self.action_conditional, action_size=self.action_size,
                                           device=device).to(self.device)

        constraints = torch.zeros((self.phycell_channels, *self.phycell_kernel_size))
        ind = 0
        for i in range(0, self.phycell_kernel_size[0]):
            for j in range(0, self.phycell_kernel_size[1]):
                constraints[ind, i, j] = 1
                ind += 1
        # (what the moment-loss kernel builds on the fly; kept for the reference's attribute, out of the state_dict like there)
        self.register_buffer("constraints", constraints.to(self.device), persistent=False)
        for m in self.modules():
            if hasattr(type(m), "precision") and m is not self:
                m.precision = self.cell_precision

    # ---- the step schedule ---------------------------------------------------------------------------------------------------------
    def _encode(self, frames):
        """frames [N,C,H,W] -> (input_phys, input_conv), each [N,64,h,w] channels-last."""
        e = self.encoder_E(frames)
        return self.encoder_Ep(e), self.encoder_Er(e)

    def _decode_logits(self, phys, conv):
        return self.decoder_D(self.decoder_Dr(conv, residual=self.decoder_Dp(phys)))

    def forward(self, x, pred_frames=1, **kwargs):
        train = kwargs.get("train", False)
        teacher_forcing = kwargs.get("teacher_forcing", False) and train
        context_frames = x.shape[1] - pred_frames if train else x.shape[1]
        if context_frames < 1:
            raise ValueError(f"PhyDNet: {x.shape[1]} input frames leave no context frame for {pred_frames} predictions in training")
        b = x.shape[0]
        n_steps = context_frames - 1 + pred_frames
        empty_actions = torch.zeros(b, n_steps, device=x.device)
        actions = kwargs.get("actions", empty_actions)
        if self.action_conditional:
            if actions is None or actions.equal(empty_actions) or actions.shape[-1] != self.action_size:
                raise ValueError("Given actions are None or of the wrong size!")
        act = (lambda s: actions[:, s]) if self.action_conditional else (lambda s: None)

        # every frame whose encoder input is known before the recurrence starts, encoded in one batch (frame-major)
        n_known = context_frames + (pred_frames - 1 if teacher_forcing else 0)
        known = x[:, :n_known].transpose(0, 1).reshape(n_known * b, *x.shape[2:])
        phys_all, conv_all = self._encode(known)

        first_out = 0 if train else context_frames - 1      # step whose output is result frame 0
        n_out = n_steps - first_out
        grad = torch.is_grad_enabled()
        result = None if grad else torch.empty(b, n_out, *x.shape[2:], device=x.device)
        parts, deferred = [], []                            # (train) per-step outputs (time order); steps decoded after the loop
        nxt = None
        for s in range(n_steps):
            if s < n_known:
                phys_in, conv_in = phys_all[s * b:(s + 1) * b], conv_all[s * b:(s + 1) * b]
            else:
                phys_in, conv_in = self._encode(nxt)
            out1, _ = self.phycell(phys_in, act(s), s == 0)
            _, out2 = self.convcell(conv_in, act(s), s == 0)
            if s < first_out:
                continue
            if n_known <= s + 1 < n_steps:
                # an autoregressive step: its frame is the next step's input
                self._flush(deferred, parts, result, first_out)
                frame = phy_ops.sigmoid_head(self._decode_logits(out1[-1], out2[-1]), 1, out=result, t0=s - first_out)
                parts.append(frame)
                nxt = frame[:, 0]
            else:
                deferred.append((s, out1[-1], out2[-1]))
        self._flush(deferred, parts, result, first_out)
        out_frames = result if result is not None else (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1))

        if train:
            moment = phy_ops.moment_loss(self.phycell.cell_list[0].F.conv1.weight, self.moment_loss_scale)
            model_losses = {"moment regularization loss": moment}
        else:
            model_losses = None
        return out_frames, model_losses

    def _flush(self, deferred, parts, result, first_out):
        """Decodes the deferred steps (consecutive) as one batch into their result slots."""
        if not deferred:
            return
        k = len(deferred)
        phys = torch.cat([d[1] for d in deferred], dim=0) if k > 1 else deferred[0][1]
        conv = torch.cat([d[2] for d in deferred], dim=0) if k > 1 else deferred[0][2]
        parts.append(phy_ops.sigmoid_head(self._decode_logits(phys, conv), k, out=result, t0=deferred[0][0] - first_out))
        deferred.clear()

    def pred_1(self, x, **kwargs):
        return self(x, pred_frames=1, **kwargs)[0].squeeze(dim=1)

    # ---- training ------------------------------------------------------------------------------------------------------------------
    def _teacher_forcing_draw(self):
        """The reference's schedule (phydnet.py train_iter): teacher forcing with probability max(0, 1 - epoch * teacher_forcing_decay)."""
        return random.random() < np.maximum(0, 1 - self.training_epoch * self.teacher_forcing_decay)

    def training_loss(self, inp, targets, pred_frames, loss_provider, teacher_forcing=None, **fwd_kwargs):
        """Loss of ONE training iteration of the reference (phydnet.py train_iter), for train_iter and train.DataParallelTrainer alike.

        `inp` holds the context frames and `targets` the `pred_frames` frames that follow them (what `unpack_data` returns); the step runs
        the training forward over their concatenation and takes the image losses against every frame from the second one on, plus the
        moment loss. `teacher_forcing=None` draws it from the schedule at `training_epoch`, which train_iter sets (a caller that drives
        the model itself, such as the data-parallel trainer, sets `model.training_epoch` per epoch)."""
        fwd_kwargs.pop("train", None)
        if targets is None or targets.dim() != inp.dim() or targets.shape[1] != pred_frames or targets.shape[0] != inp.shape[0]:
            raise ValueError(f"PhyDNet.training_loss: targets must hold the {pred_frames} frames that follow the context frames of `inp`, "
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
            inp, targets, actions = self.unpack_data(data, config)
            total = self.training_loss(inp, targets, config["pred_frames"], loss_provider, actions=actions)
            optimizer.zero_grad()
            total.backward()
            optimizer.step()
            if hasattr(loop, "set_postfix"):
                loop.set_postfix(loss=total.item())
