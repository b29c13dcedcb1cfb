"""DreamBooth PSO step for SDXL-Turbo (BASELINE config 5), MI355X-native.

Reference: DB = personalization/train_pso_sdxl_turbo_dreambooth.py, the micro-step DB:1720-1964 with the recipe of
personalization/scripts/pso_dog.sh (EDM-style epsilon training, loss "pso_db", beta 5, prior weight 0.5, rank 16):

  pixel_values = [instances; negatives]                                  DB:1731
  x0     = vae.encode(pixel_values).latent_dist.sample() * scaling       DB:1750-1753
  noise  = one draw shared by both halves                                DB:1763
  t      = stride * (randint % 4) + stride - 1  in {249,499,749,999}     DB:1769-1777 (turbo branch), same for both
  noisy  = x0 + noise * sigma(t) ; unet_in = noisy / sqrt(sigma^2 + 1)   DB:1787-1796
  eps    = unet(unet_in, t, prompt_embeds x2, {time_ids, text_embeds})   DB:1815-1825
  loss   = fused DreamBooth PSO loss (csrc/db_loss.hip)                  DB:1847-1935
  backward -> LoRA grads ; every gradient_accumulation_steps: clip + AdamW   DB:1953-1964

Here the VAE encoder, the UNet forward/backward and the loss all run on libpso_amd; for loss_type "pso" the reference
eps (adapters disabled, DB:1894-1920) comes from the same paired UNet pass as the policy eps.  No host sync.

Under the f16 library (the recipes' own --mixed_precision="fp16") the trainer needs a loss scaler (loss_scale=): the
backward runs on loss * S / gas and the shared optimizer step unscales, skips a non-finite step and backs the scale
off.  The front end is fp32 in the reference as well: the recipes name a VAE, so the latents are not cast to the
weight dtype (DB:1754-1755) and the VAE stays fp32 (DB:1293); noise, add_noise, the sigmas and the EDM
preconditioning are fp32 -- what prepare_inputs and db_loss.hip compute.
"""

import warnings

import torch

from . import _lib
from . import kernels as K
from .amp import DeviceLossScaler, LossScaler, make_scaler
from .schedulers import EulerDiscreteScheduler, db_distill_timesteps
from .trainer import (EMA_ARG_KEYS, LastLr, OptStep, check_ema_live, init_ema, init_lr_schedule,
                      init_optimizer_state, lora_optimizer_step)


class DreamBoothPSOTrainer:
    opt_step = OptStep()
    last_lr = LastLr()

    def __init__(self, unet, vae, loss_type="pso_db", beta_pso=5.0, neg_defactor=0.1, prior_loss_weight=0.5,
                 distill_train_timesteps=4, learning_rate=2e-4, betas=(0.9, 0.999), adam_weight_decay=1e-4,
                 adam_epsilon=1e-8, max_grad_norm=1.0, gradient_accumulation_steps=4, process_group=None,
                 loss_scale=None, use_8bit_adam=False, optimizer="adamw", prodigy_beta3=None, prodigy_decouple=True,
                 prodigy_use_bias_correction=False, prodigy_safeguard_warmup=False, prodigy_d0=1e-6,
                 prodigy_d_coef=1.0, prodigy_growth_rate=float("inf"), lr_scheduler="constant", lr_warmup_steps=0,
                 max_train_steps=None, lr_num_cycles=1, lr_power=1.0, use_ema=False, ema_decay=0.9999,
                 ema_min_decay=0.0, ema_update_after_step=0, ema_use_warmup=False, ema_inv_gamma=1.0, ema_power=2 / 3):
        """Defaults: DB argparse defaults (DB:636-674, 757-777) overridden by the recipe scripts/pso_dog.sh.
        loss_scale: None | float (initial scale) | amp.LossScaler | amp.DeviceLossScaler -- fp16 training under the
        f16 library, which refuses to train without one; the bf16 library takes none.  use_8bit_adam: the script's
        --use_8bit_adam (DB:630), the blockwise 8-bit AdamW as in PSOTrainer.  optimizer: "adamw" or "prodigy"
        (--optimizer, DB:622-627; case-insensitive) with the prodigy_* arguments of PSOTrainer; Prodigy wants a
        learning_rate around 1.0 and reads betas, adam_weight_decay and adam_epsilon as the diffusers script does.
        lr_scheduler / lr_warmup_steps / max_train_steps / lr_num_cycles / lr_power: the script's get_scheduler call
        (DB:1614-1621), stepped once per applied optimizer step (DB:1962-1963); "constant" builds no schedule
        (self.lr_schedule is None) whatever lr_warmup_steps says, as diffusers' constant kind ignores it.
        use_ema / ema_*: diffusers' --use_ema with the EMAModel arguments, as in PSOTrainer; off, self.ema is None."""
        if loss_type not in ("pso", "pso_db"):
            raise ValueError(f"Unknown loss type {loss_type}")  # DB:1929
        self.scaler = make_scaler(loss_scale)
        if self.scaler is None:
            # without a loss scaler the f16 library would train fp16 unscaled
            _lib.require_bf16("DreamBooth PSO training (DreamBoothPSOTrainer) without loss_scale=")
        elif _lib.ELEM_DTYPE != torch.float16:
            raise ValueError("loss_scale is for fp16 training (PSO_LIB=f16, libpso_amd_f16.so); the loaded library "
                             f"computes in {_lib.ELEM_DTYPE}")
        self.unet, self.vae = unet, vae
        self.loss_type = loss_type
        self.lt = K.DB_SIGMOID if loss_type == "pso" else K.DB_HINGE
        self.beta, self.nd, self.prior_w = float(beta_pso), float(neg_defactor), float(prior_loss_weight)
        self.distill_steps = distill_train_timesteps
        self.lr, self.betas, self.wd, self.adam_eps = learning_rate, betas, adam_weight_decay, adam_epsilon
        self.max_grad_norm = max_grad_norm
        self.gas = gradient_accumulation_steps
        self.pg = process_group
        self.sched = EulerDiscreteScheduler()
        st = unet.lora
        init_optimizer_state(self, unet, optimizer=optimizer, use_8bit_adam=use_8bit_adam,
                             prodigy_beta3=prodigy_beta3, prodigy_decouple=prodigy_decouple,
                             prodigy_use_bias_correction=prodigy_use_bias_correction,
                             prodigy_safeguard_warmup=prodigy_safeguard_warmup, prodigy_d0=prodigy_d0,
                             prodigy_d_coef=prodigy_d_coef, prodigy_growth_rate=prodigy_growth_rate)
        init_lr_schedule(self, lr_scheduler, lr_warmup_steps, max_train_steps, lr_num_cycles, lr_power)
        init_ema(self, unet, use_ema, ema_decay, ema_min_decay, ema_update_after_step, ema_use_warmup, ema_inv_gamma,
                 ema_power)
        self.clip_buf = torch.zeros(2, device=st.master.device, dtype=torch.float32)
        self.opt_step = 0
        self.n_micro = 0
        self.loss_hist = []
        self.auto_step = True

    @classmethod
    def from_args(cls, unet, vae, args, process_group=None, loss_scale=None, allow_prodigy=False,
                  allow_lr_schedule=False, allow_dora=False):
        """Build from the reference script's argparse namespace (DB:parse_args).  Read: loss_type, beta_pso,
        neg_defactor, prior_loss_weight, distill_train_timesteps, learning_rate, adam_beta1 / adam_beta2 /
        adam_weight_decay / adam_epsilon, max_grad_norm, gradient_accumulation_steps, use_8bit_adam, mixed_precision,
        optimizer ("AdamW" or "prodigy"; any other name warns and becomes AdamW, DB:1479-1484) and, for Prodigy,
        prodigy_beta3 / prodigy_decouple / prodigy_use_bias_correction / prodigy_safeguard_warmup (DB:641-673), which
        also warns for a learning_rate <= 0.1 and ignores use_8bit_adam with a warning (DB:1486-1490).  Prodigy
        trains with allow_prodigy=True only: without it optimizer="prodigy" raises ValueError as it always has, so a
        caller that relied on the refusal keeps it.  The same holds for the learning-rate schedule: with
        allow_lr_schedule=True lr_scheduler, lr_warmup_steps (script default 500), max_train_steps, lr_num_cycles and
        lr_power are read and the schedule is built (DB:1614-1621; the script's own defaults -- "constant" with a
        warm-up of 500 that the constant kind ignores -- give none); without it anything but "constant" with zero
        warm-up raises ValueError as it always has.  And for --use_dora (DB:741): with allow_dora=True it is accepted
        if and only if the UNet's adapter is a DoRA one (unet.lora.dora; add_adapter(cfg, allow_dora=True)) -- a
        mismatch in either direction raises ValueError naming use_dora -- and without it use_dora raises as it always
        has;
        use_ema and ema_decay / ema_min_decay / ema_update_after_step / ema_use_warmup / ema_inv_gamma / ema_power are
        read when the namespace carries them (the reference script has no such flags: absent means no EMA);
        a field the namespace does not carry counts as the script's default.  Flags that ask for training this
        trainer does not implement raise ValueError naming the flag (unet.check_lora_config's rule) instead of
        training something else.
        Precision: the f16 library runs mixed_precision="fp16" only and trains with `loss_scale` (default: a host
        amp.LossScaler()); the bf16 library keeps its documented substitute -- bf16 arithmetic, no scaler -- whatever
        mixed_precision says."""
        def get(name, default):
            return getattr(args, name, default)

        optimizer = str(get("optimizer", "AdamW")).lower()
        if optimizer not in ("adamw", "prodigy"):  # the script's own fallback, DB:1479-1484
            warnings.warn(f"Unsupported choice of optimizer: {get('optimizer', None)!r}. Supported optimizers include "
                          "[adamW, prodigy]. Defaulting to adamW")
            optimizer = "adamw"
        use_8bit_adam = bool(get("use_8bit_adam", False))
        prodigy = {}
        if optimizer == "prodigy":
            if not allow_prodigy:
                raise ValueError("--optimizer='prodigy' trains only on request: pass from_args(..., "
                                 "allow_prodigy=True).  The reference script builds no optimizer for it (DB:1492-1510), "
                                 "so a namespace that carries it was never a working run there")
            if use_8bit_adam:  # DB:1486-1490
                warnings.warn("use_8bit_adam is ignored when optimizer is not set to 'AdamW'. Optimizer was set to "
                              "prodigy")
                use_8bit_adam = False
            if get("learning_rate", 1e-4) <= 0.1:
                warnings.warn("Learning rate is too low. When using prodigy, it's generally better to set it around "
                              "1.0")
            # the script's defaults, DB:641-673: beta3 None (sqrt(beta2)), the three switches on
            prodigy = dict(prodigy_beta3=get("prodigy_beta3", None),
                           prodigy_decouple=bool(get("prodigy_decouple", True)),
                           prodigy_use_bias_correction=bool(get("prodigy_use_bias_correction", True)),
                           prodigy_safeguard_warmup=bool(get("prodigy_safeguard_warmup", True)))
        for flag in ("train_text_encoder", "with_prior_preservation", "use_dora"):
            if get(flag, False) and not (flag == "use_dora" and allow_dora):
                raise ValueError(f"--{flag} is not implemented (the recipes under personalization/scripts leave it off)")
        if allow_dora:
            # the script hands use_dora to LoraConfig (DB:1321): the UNet's adapter must be the kind the flag names
            want, have = bool(get("use_dora", False)), bool(getattr(unet.lora, "dora", False))
            if want != have:
                raise ValueError(f"--use_dora={want} but the UNet carries a {'DoRA' if have else 'plain LoRA'} adapter: "
                                 "add it with LoraConfig(use_dora=args.use_dora) and add_adapter(..., allow_dora=True)")
        if not get("do_edm_style_training", False):
            raise ValueError("--do_edm_style_training is required: only the EDM-style epsilon training of the recipes "
                             "(DB:1787-1796) is implemented")
        sched = get("lr_scheduler", "constant")
        schedule = {}
        if allow_lr_schedule:
            schedule = dict(lr_scheduler=sched, lr_warmup_steps=get("lr_warmup_steps", 500),
                            max_train_steps=get("max_train_steps", None), lr_num_cycles=get("lr_num_cycles", 1),
                            lr_power=get("lr_power", 1.0))
        else:
            if sched != "constant":
                raise ValueError(f"--lr_scheduler={sched!r} is not implemented (constant only)")
            if get("lr_warmup_steps", 500) != 0:
                raise ValueError(f"--lr_warmup_steps={get('lr_warmup_steps', 500)!r} is not implemented: the constant "
                                 "schedule here has no warm-up (the recipes pass 0)")
        mp = get("mixed_precision", None)
        if _lib.ELEM_DTYPE == torch.float16:
            if mp != "fp16":
                raise ValueError(f"the f16 library (PSO_LIB=f16) trains --mixed_precision=fp16 only, got {mp!r}: "
                                 "unset PSO_LIB for the bf16 library")
            if loss_scale is None:
                loss_scale = LossScaler()
        elif loss_scale is not None:
            raise ValueError("loss_scale is for fp16 training (PSO_LIB=f16, libpso_amd_f16.so); the loaded library "
                             f"computes in {_lib.ELEM_DTYPE}")
        return cls(unet, vae, loss_type=get("loss_type", "sigmoid"), beta_pso=get("beta_pso", 200),
                   neg_defactor=get("neg_defactor", 0.1), prior_loss_weight=get("prior_loss_weight", 1.0),
                   distill_train_timesteps=get("distill_train_timesteps", 4),
                   learning_rate=get("learning_rate", 1e-4), betas=(get("adam_beta1", 0.9), get("adam_beta2", 0.999)),
                   adam_weight_decay=get("adam_weight_decay", 1e-4), adam_epsilon=get("adam_epsilon", 1e-8),
                   max_grad_norm=get("max_grad_norm", 1.0),
                   gradient_accumulation_steps=get("gradient_accumulation_steps", 1), process_group=process_group,
                   loss_scale=loss_scale, use_8bit_adam=use_8bit_adam, optimizer=optimizer, **prodigy, **schedule,
                   **{k: getattr(args, k) for k in EMA_ARG_KEYS if hasattr(args, k)})

    @property
    def loss_scale(self):
        """The factor on the loss in backward (1.0 without a scaler); with a DeviceLossScaler this reads the device."""
        return 1.0 if self.scaler is None else self.scaler.scale

    def prepare_inputs(self, pixel_values, generator=None):
        """DB:1731-1796 on device: latents, shared noise, distilled timesteps, EDM-preconditioned UNet input.
        pixel_values [2B,3,H,W] in [-1,1] (instances first).  Returns a dict of NHWC tensors."""
        dev = pixel_values.device
        B2 = pixel_values.shape[0]
        B = B2 // 2
        mo = self.vae.encode_nhwc(pixel_values)                                   # [2B,h,w,8] fp32
        L = self.vae.cfg.latent_channels
        mean, logvar = mo[..., :L], mo[..., L:].clamp(-30.0, 20.0)
        z = torch.randn(mean.shape, device=dev, generator=generator)
        x0 = ((mean + torch.exp(0.5 * logvar) * z) * self.vae.config.scaling_factor).contiguous()
        noise = torch.randn((B,) + tuple(x0.shape[1:]), device=dev, generator=generator).repeat(2, 1, 1, 1)
        raw = torch.randint(0, self.sched.num_train_timesteps, (B,), device=dev, generator=generator)
        t = db_distill_timesteps(raw, self.distill_steps, self.sched.num_train_timesteps).repeat(2)
        sigma = self.sched.sigma_at(t)
        s4 = sigma.view(-1, 1, 1, 1)
        noisy = (x0 + noise * s4).contiguous()
        unet_in = K.cast_f32_bf16(noisy / torch.sqrt(s4 * s4 + 1.0))
        return dict(x0=x0, noisy=noisy, sigma=sigma.contiguous(), t=t.float(), unet_in=unet_in)

    def micro_step(self, pixel_values, prompt_embeds, pooled, time_ids, generator=None):
        """One DreamBooth PSO micro-step (DB:1720-1964).  prompt_embeds [B,77,D], pooled [B,Dp], time_ids [B,6] are
        the instance prompt's; both halves use them (DB:1804, 1816-1818).  Returns the loss (device scalar)."""
        check_ema_live(self, "micro_step")
        inp = self.prepare_inputs(pixel_values, generator)
        enc = prompt_embeds.repeat(2, 1, 1)
        pl = pooled.repeat(2, 1)
        tid = time_ids.repeat(2, 1)
        u = self.unet
        u.enable_adapters()
        paired = self.loss_type == "pso"
        eps, rt = u.forward_nhwc(inp["unet_in"], inp["t"], enc, pl, tid, save=True, paired_ref=paired)
        n = inp["unet_in"].shape[0]
        eps_pol = eps[:n]
        eps_ref = eps[n:] if paired else None
        ws = K.db_loss_ws(n // 2, eps_pol[0].numel(), eps.device)
        loss, _, _ = K.db_loss_fwd(self.lt, eps_pol, inp["noisy"], inp["x0"], inp["sigma"], self.beta, self.nd,
                                   self.prior_w, ws, eps_ref=eps_ref)
        # accelerator.backward divides by gradient_accumulation_steps
        if isinstance(self.scaler, DeviceLossScaler):  # loss * S / gas, S read on the device
            deps = K.db_loss_bwd(self.lt, eps_pol, inp["noisy"], inp["x0"], inp["sigma"], self.beta, self.nd,
                                 self.prior_w, ws, grad_out=self.scaler.scale_word, grad_scale=1.0 / self.gas)
        else:
            deps = K.db_loss_bwd(self.lt, eps_pol, inp["noisy"], inp["x0"], inp["sigma"], self.beta, self.nd,
                                 self.prior_w, ws, grad_scale=1.0 / self.gas * self.loss_scale)
        u.backward_nhwc(deps, rt)
        self.loss_hist.append(loss)
        self.n_micro += 1
        if self.auto_step and self.n_micro % self.gas == 0:
            self.optimizer_step()
        return loss

    def optimizer_step(self):
        lora_optimizer_step(self)
