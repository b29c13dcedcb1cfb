"""LoRA checkpoint interchange in the diffusers format the reference writes and reads.

* `save_lora_weights(output_dir, unet_lora_layers)` -- `StableDiffusionXLLoraLoaderMixin.save_lora_weights`
  as used by the save hook `T:361-379`: `pytorch_lora_weights.safetensors`, keys `unet.<module>.lora.{down,up}.weight`
  (peft `lora_A/lora_B` renamed by `convert_state_dict_to_diffusers`).
* `lora_state_dict(input_dir)` / `load_lora_into_unet(sd, network_alphas, unet)` -- the load hook `T:381-395`
  (and the consumers `T:138`, `evaluate_sdxl_dmd2.py:194`); accepts diffusers (`lora.down/up`) or peft
  (`lora_A/lora_B`) naming, with or without the `unet.` prefix.
* `save_state(trainer, dir)` / `load_state(trainer, dir)` -- resume (`T:886-890`, `accelerator.save_state`): the
  LoRA file plus the AdamW moments and step count (`optimizer.safetensors`).  8-bit AdamW checkpoints carry the
  per-tensor block table (round 4 on); an older checkpoint without one (uniform 2048-element blocks over the flat
  buffer) is re-quantised into the per-tensor layout on load, with a warning.  A trainer with a loss scaler
  (`amp.LossScaler` or `amp.DeviceLossScaler`, fp16 training) also writes the scaler's `state_dict()` under the
  additive key `loss_scaler` of `pso_state.json`; a checkpoint without it loads as before and keeps the trainer's
  scaler as constructed.  A Prodigy trainer (`optimizer="prodigy"`) writes `p0`, `exp_avg`, `exp_avg_sq`, `s` and
  the scalar state block `prodigy_state` instead, and `pso_state.json` names the optimizer under the additive key
  `optimizer`; loading a checkpoint of the other optimizer raises `KeyError`.  A trainer with a learning-rate schedule
  writes its `state_dict()` under the additive key `lr_schedule`; the position in the schedule is `opt_step` and needs
  no field of its own.  A DoRA adapter (`LoraState.dora`) adds one `unet.<module>.lora_magnitude_vector.weight` per
  module to the LoRA file (peft 0.11's key; the converters below leave it as it is, and the bare
  `lora_magnitude_vector` of older peft releases loads too), and its moments lie in the flat optimizer buffers like
  any other tensor's.  A file with magnitudes does not load into a plain-LoRA UNet, nor one without into a DoRA UNet:
  both raise `ValueError` naming `lora_magnitude_vector`.  On load the trainer's own schedule wins: one that differs from the checkpoint's (or a
  checkpoint with a schedule into a trainer without) warns; a checkpoint without the key loads as before.
  A trainer with an EMA of its weights (`use_ema`, `ema.EMAModel`) writes the shadow as a LoRA file of its own,
  `pytorch_lora_weights_ema.safetensors`, next to the live one -- the same key layout (magnitudes included under
  DoRA), so `lora_state_dict(dir, weight_name=...)` + `load_lora_into_unet` load it like any adapter -- and the EMA's
  scalars under the additive key `ema`; loading restores both, so a resumed run continues bit for bit.  A checkpoint
  without `ema` into a trainer with one raises `KeyError`; one with `ema` into a trainer without loads the rest and
  warns.
"""
import json
import os
import warnings

import torch
from safetensors.torch import load_file, save_file

LORA_WEIGHT_NAME = "pytorch_lora_weights.safetensors"
EMA_LORA_WEIGHT_NAME = "pytorch_lora_weights_ema.safetensors"
OPT_NAME = "optimizer.safetensors"


def peft_to_diffusers(sd):
    """convert_state_dict_to_diffusers for a peft LoRA state dict: `.lora_A.` -> `.lora.down.`, `.lora_B.` -> `.lora.up.`
    (DoRA's `.lora_magnitude_vector.` keys pass through unchanged)"""
    out = {}
    for k, v in sd.items():
        out[k.replace(".lora_A.", ".lora.down.").replace(".lora_B.", ".lora.up.")] = v
    return out


def diffusers_to_peft(sd):
    out = {}
    for k, v in sd.items():
        if k.startswith("unet."):
            k = k[len("unet."):]
        out[k.replace(".lora.down.", ".lora_A.").replace(".lora.up.", ".lora_B.")] = v
    return out


def get_peft_model_state_dict(unet):
    return unet.lora.state_dict_peft()


def save_lora_weights(output_dir, unet_lora_layers, weight_name=LORA_WEIGHT_NAME):
    os.makedirs(output_dir, exist_ok=True)
    packed = {f"unet.{k}": v.detach().float().contiguous().cpu() for k, v in unet_lora_layers.items()}
    save_file(packed, os.path.join(output_dir, weight_name), metadata={"format": "pt"})


def lora_state_dict(input_dir, weight_name=LORA_WEIGHT_NAME):
    path = input_dir if input_dir.endswith(".safetensors") else os.path.join(input_dir, weight_name)
    return load_file(path), None


def load_lora_into_unet(state_dict, network_alphas, unet):
    """Copy a LoRA state dict into the unet's adapter (ranks must match; network_alphas other than None/rank are
    folded into B as alpha/r, like peft's scaling)."""
    sd = diffusers_to_peft(state_dict)
    st = unet.lora
    missing = [n for n in st.adapter_names() if f"{n}.lora_A.weight" not in sd or f"{n}.lora_B.weight" not in sd]
    if missing:
        raise KeyError(f"LoRA state dict lacks {len(missing)} adapters, e.g. {missing[0]}")
    for n in st.adapter_names():
        A, B = sd[f"{n}.lora_A.weight"], sd[f"{n}.lora_B.weight"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != st.r or B.shape[1] != st.r:
            raise ValueError(f"LoRA state dict has rank {A.shape[0] if A.dim() == 2 else tuple(A.shape)} adapters "
                             f"({n}: lora_A {tuple(A.shape)}, lora_B {tuple(B.shape)}), the unet's adapter has rank "
                             f"{st.r}: add the adapter with LoraConfig(r=<the file's rank>)")
    dev = st.master.device
    st.load_peft({k: v.to(dev, torch.float32) for k, v in sd.items()})


def load_lora_weights(unet, input_dir, weight_name=LORA_WEIGHT_NAME):
    """The pipeline's `load_lora_weights(dir, weight_name=...)` for this UNet: lora_state_dict + load_lora_into_unet.
    weight_name=EMA_LORA_WEIGHT_NAME loads the averaged adapter that save_state writes for a trainer with use_ema."""
    sd, alphas = lora_state_dict(input_dir, weight_name=weight_name)
    load_lora_into_unet(sd, alphas, unet)


def save_state(trainer, output_dir):
    unet = trainer.unet
    ema = getattr(trainer, "ema", None)
    if ema is not None:
        if ema.swapped:
            raise RuntimeError("save_state while the EMA weights are swapped in: restore() the live weights first")
        save_lora_weights(output_dir, peft_to_diffusers(ema.state_dict_peft()), weight_name=EMA_LORA_WEIGHT_NAME)
    save_lora_weights(output_dir, peft_to_diffusers(get_peft_model_state_dict(unet)))
    a8 = getattr(trainer, "adam8", None)
    pro = getattr(trainer, "prodigy", None)
    if pro is not None:  # Prodigy: p0, the moments, s and the scalar state block as they stand
        opt = {k: v.cpu() for k, v in pro.tensors().items()}
    elif a8 is not None:  # 8-bit AdamW state as it stands (codes + block absmax): a resume continues bit for bit
        opt = {k: v.cpu() for k, v in a8.tensors().items()}
    else:
        opt = {"exp_avg": trainer.exp_avg.cpu(), "exp_avg_sq": trainer.exp_avg_sq.cpu()}
    save_file(opt, os.path.join(output_dir, OPT_NAME),
              metadata={"step": str(trainer.opt_step), "n_micro": str(trainer.n_micro)})
    with open(os.path.join(output_dir, "pso_state.json"), "w") as f:
        meta = {"opt_step": trainer.opt_step, "n_micro": trainer.n_micro, "rank": unet.lora.r,
                "optimizer": "prodigy" if pro is not None else "adamw8bit" if a8 is not None else "adamw"}
        scaler = getattr(trainer, "scaler", None)
        if scaler is not None:
            meta["loss_scaler"] = scaler.state_dict()
        sched = getattr(trainer, "lr_schedule", None)
        if sched is not None:
            meta["lr_schedule"] = sched.state_dict()
        if ema is not None:
            meta["ema"] = ema.scalars()
        json.dump(meta, f)


def load_state(trainer, input_dir):
    with open(os.path.join(input_dir, "pso_state.json")) as f:
        meta = json.load(f)
    ema = getattr(trainer, "ema", None)
    if ema is not None:
        if "ema" not in meta:
            raise KeyError("checkpoint holds no EMA state; this trainer averages its weights (use_ema=True)")
        if ema.swapped:
            raise RuntimeError("load_state while the EMA weights are swapped in: restore() the live weights first")
    elif "ema" in meta:
        warnings.warn("checkpoint was written with an EMA of the weights (use_ema); this trainer keeps none: "
                      f"{EMA_LORA_WEIGHT_NAME} and the EMA counters are not loaded")
    sd, alphas = lora_state_dict(input_dir)
    load_lora_into_unet(sd, alphas, trainer.unet)
    if ema is not None:
        ema.load_peft(diffusers_to_peft(lora_state_dict(input_dir, weight_name=EMA_LORA_WEIGHT_NAME)[0]))
        ema.load_scalars(meta["ema"])
    opt = load_file(os.path.join(input_dir, OPT_NAME))
    a8 = getattr(trainer, "adam8", None)
    pro = getattr(trainer, "prodigy", None)
    if pro is None and "prodigy_state" in opt:
        raise KeyError("checkpoint holds Prodigy state; this trainer runs AdamW (optimizer='adamw')")
    if pro is not None:
        if "prodigy_state" not in opt:
            raise KeyError("checkpoint holds AdamW state; this trainer runs Prodigy (optimizer='prodigy')")
        for k, t in pro.tensors().items():
            t.copy_(opt[k])
    elif a8 is not None:
        if "exp_avg_q" not in opt:
            raise KeyError("checkpoint holds fp32 AdamW state; this trainer runs the 8-bit AdamW (use_8bit_adam)")
        mine = a8.tensors()
        if "block_table" in mine and "block_table" not in opt:
            # a checkpoint of rounds <= 3: uniform 2048-element blocks over the whole flat buffer.  Its moments are
            # dequantised in that layout and re-quantised into the per-tensor blocks (lossy only in the code
            # rounding of the new blocks)
            warnings.warn("8-bit AdamW checkpoint without a block table (uniform blocks, older format): its moments "
                          "are re-quantised into the per-tensor block layout")
            from . import kernels as K
            old = K.Adam8State(a8.n, a8.qm.device)
            for k, t in old.tensors().items():
                t.copy_(opt[k])
            a8.load_dense(*old.dequant())
        elif ("block_table" in mine) != ("block_table" in opt) or (
                "block_table" in opt and not torch.equal(opt["block_table"], mine["block_table"].cpu())):
            raise KeyError("checkpoint's 8-bit AdamW block layout differs from this trainer's parameter tensors")
        else:
            for k, t in mine.items():
                if k != "block_table":
                    t.copy_(opt[k])
    else:
        if "exp_avg" not in opt:
            raise KeyError("checkpoint holds 8-bit AdamW state; this trainer runs fp32 AdamW")
        trainer.exp_avg.copy_(opt["exp_avg"])
        trainer.exp_avg_sq.copy_(opt["exp_avg_sq"])
    scaler = getattr(trainer, "scaler", None)
    if scaler is not None and "loss_scaler" in meta:
        scaler.load_state_dict(meta["loss_scaler"])
    trainer.opt_step, trainer.n_micro = int(meta["opt_step"]), int(meta["n_micro"])
    if "lr_schedule" in meta:
        sched = getattr(trainer, "lr_schedule", None)
        mine = None if sched is None else sched.state_dict()
        if mine != meta["lr_schedule"]:
            warnings.warn(f"checkpoint was written with the learning-rate schedule {meta['lr_schedule']}, this trainer "
                          f"runs {mine if mine is not None else 'a constant rate'}: the trainer's is kept, continuing "
                          f"at optimizer step {trainer.opt_step}")
    if getattr(trainer, "lr_word", None) is not None:  # last_lr reads the word: the resumed step's lr
        from .trainer import sync_lr_word
        sync_lr_word(trainer)
