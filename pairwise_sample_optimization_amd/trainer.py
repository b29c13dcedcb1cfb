"""The online PSO epoch for timestep-distilled SDXL, MI355X-native: paired on-policy sampling, trajectory buffer +
shuffles, the (pair-batch, transition) micro-step and the optimizer step.

Reference loop (`T` = human_preference_tuning/train_online_pso_sdxl_turbo.py, `D` = ..._dmd2.py):
  SAMPLING  T:554-673 / D:557-679  two independent trajectories per prompt through the distilled UNet, rewards
  BUFFER    T:610-666,714-749       stack (B, 2, T, ...); per inner epoch permute pairs and, independently per pair,
                                    the transition order (same for both members)
  MICRO     T:771-861 / D:773-864   2 policy UNet fwd (LoRA on) + 2 reference fwd (adapters off) + 4 step log-probs
                                    + clipped pairwise loss + backward; grads accumulate over gas*T micro-steps
  SYNC      T:857-861               DDP all-reduce, clip_grad_norm_(1.0), optimizer.step, zero_grad

Here every per-element operation runs in libpso_amd; the micro-step issues no host synchronisation (the reference
syncs 4x in turbo_step_with_logprob's `.item()` lookups and once in `accelerator.gather(loss).item()`).  The two
members of every pair ride in ONE UNet batch (image order 2p + k), policy and reference forwards share the frozen
weights, the loss kernel consumes the bf16 NHWC eps directly and emits d loss / d eps for the hand-written UNet
backward, which accumulates LoRA grads into the flat all-reduce bucket.
"""
import gc
import math
from types import SimpleNamespace

import torch
import torch.distributed as dist

import os

from . import _lib
from . import kernels as K
from . import pso_core
from .amp import DeviceLossScaler, LossScaler, make_scaler
from .lr_schedule import make_lr_schedule
from ._lib import MODE_TURBO, MODE_DMD
from .schedulers import EulerAncestralDiscreteScheduler, LCMScheduler, dmd_distill_timesteps

# full-UNet mode: the frozen reference pass on a stream of its own (PSO_REF_STREAM=0 keeps it in line, A/B knob)
_REF_STREAM = os.environ.get("PSO_REF_STREAM", "1") == "1"
_GC_PAUSE = os.environ.get("PSO_GC_PAUSE", "1") == "1"  # train_epoch: cyclic GC paused (A/B knob)
_REF_STREAMS = {}


def _ref_stream():
    """ONE reference-pass stream per device for the process (the caching allocator keeps freed blocks per stream)."""
    dev = torch.cuda.current_device()
    st = _REF_STREAMS.get(dev)
    if st is None:
        st = _REF_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return st


ELEM = _lib.ELEM_DTYPE  # the loaded library's 16-bit element type: bf16, or fp16 under PSO_LIB=f16


def compute_time_ids(size, crop=0, device=None):
    """T:324-332 (512) / D:347-355 (1024): [orig_h, orig_w, crop_top, crop_left, target_h, target_w]."""
    return torch.tensor([[size, size, crop, crop, size, size]], dtype=torch.float32, device=device)


def shuffle_index(perm, perms, P):
    """Row indices of the shuffled, re-batched training stream (T:733-760 / D:719-753).

    perm [Bp] pair permutation, perms [Bp, T] per-row time permutation.  The reference applies `perms` after
    `samples = samples[perm]`, so shuffled row i = old pair perm[i] with time order perms[i].  Micro-step s = (batch b, step j) holds, for p < P and
    member k, buffer row ((perm[bP+p]*2 + k)*T + perms[bP+p, j]) of the [2Bp*T] latent stream.
    Returns (img_idx [nb*T*P*2], pair_img [same] rows of per-pair tensors, tsel [same] transition index)."""
    Bp, T = perms.shape
    nb = Bp // P
    dev = perm.device
    pb = torch.arange(nb, device=dev).view(nb, 1, 1, 1)
    jj = torch.arange(T, device=dev).view(1, T, 1, 1)
    pp = torch.arange(P, device=dev).view(1, 1, P, 1)
    kk = torch.arange(2, device=dev).view(1, 1, 1, 2)
    row = pb * P + pp                                         # new (shuffled) position  [nb,1,P,1]
    pair = perm[row]                                          # old pair id
    tsel = perms[row, jj]                                     # [nb,T,P,1]
    img_idx = ((pair * 2 + kk) * T + tsel).reshape(-1)
    pair_img = (pair * 2 + kk).expand(nb, T, P, 2).reshape(-1)
    tsel_i = tsel.expand(nb, T, P, 2).reshape(-1)
    return img_idx, pair_img, tsel_i


def allreduce_grads(flat, process_group=None, wire_dtype=None):
    """DDP gradient sync of the flat trained gradient in one collective (T:857 under accelerate: all-reduce SUM, then
    the mean) -- the path when no overlapped GradBuckets sync was armed (hipGraph epochs).  The 1/world factor is
    returned, not applied: the clip and AdamW kernels fold it into their gradient read.  wire_dtype=torch.bfloat16
    reduces a bf16 copy and casts the sum back (half the bytes; fp32 accumulation stays local)."""
    if not (dist.is_available() and dist.is_initialized()):
        return 1.0
    world = dist.get_world_size(process_group)
    if world == 1:
        return 1.0
    if wire_dtype is not None and wire_dtype != flat.dtype:
        t = flat.to(wire_dtype)
        dist.all_reduce(t, group=process_group)
        flat.copy_(t)
    else:
        dist.all_reduce(flat, group=process_group)
    return 1.0 / world


class GradBuckets:
    """DDP-style gradient sync overlapped with the backward (what accelerator.backward's DDP bucket hooks do on a sync
    micro-step, T:228-233,857): the flat trained gradient is cut into ~bucket_mb contiguous buckets
    along the backward's completion order (UNet2DConditionModel.grad_unit_ranges); backward_nhwc reports every
    finished unit through rt.unit_done and, as soon as a bucket's last unit is done, its all-reduce (SUM) is issued
    asynchronously -- with RCCL it runs on the communicator's own stream, ordered after the compute stream's work so
    far, beside the rest of the backward.  finish() issues whatever is left and makes the compute stream wait for
    every bucket before the clip / AdamW read the gradient.  The 1/world mean is folded into those kernels."""

    def __init__(self, unet, flat, bucket_mb=32.0, process_group=None, wire_dtype=None):
        self.flat = flat
        self.pg = process_group
        self.world = dist.get_world_size(process_group)
        # wire_dtype=torch.bfloat16: every bucket is cast to bf16 for the all-reduce and cast back into the fp32 flat
        # gradient afterwards (what DDP's bf16_compress_hook does): half the xGMI bytes -- 5.1 instead of 10.3 GB per
        # full-UNet step (C4) -- while the local accumulation over the window's micro-steps stays fp32
        self.wire_dtype = wire_dtype
        self.timing = False      # record the compute-stream stall on the outstanding buckets (bench diagnostics)
        self.exposed_ms = []     # per finish(): ms the compute stream waited for RCCL after the backward
        self._ev = None
        cap = int(bucket_mb * 1e6 / flat.element_size())
        self.buckets = []        # [(offset, numel, last unit)]
        self.unit_bucket = {}    # unit -> bucket index (every unit of the bucket)
        units = unet.grad_unit_ranges()
        cur_off, cur_n, cur_units = None, 0, []
        for unit, off, n in units:
            if cur_off is None:
                cur_off = off
            cur_n += n
            cur_units.append(unit)
            if cur_n >= cap:
                self._close(cur_off, cur_n, cur_units)
                cur_off, cur_n, cur_units = None, 0, []
        if cur_units:
            self._close(cur_off, cur_n, cur_units)
        covered = sum(n for _, n, _ in self.buckets)
        assert covered == flat.numel(), f"buckets cover {covered} of {flat.numel()} gradient elements"
        self.reset()

    def _close(self, off, n, units):
        b = len(self.buckets)
        self.buckets.append((off, n, tuple(units)))
        for u in units:
            self.unit_bucket[u] = b

    def reset(self):
        self.pending = [set(u) for _, _, u in self.buckets]
        self.works = [None] * len(self.buckets)
        self.wire = [None] * len(self.buckets)

    def _issue(self, b, side=None):
        if self.works[b] is not None:
            return
        if side is not None:
            side.join()  # LoRA dW launches on the side stream belong to this bucket
        off, n, _ = self.buckets[b]
        t = self.flat[off:off + n]
        if self.wire_dtype is not None and self.wire_dtype != t.dtype:
            t = t.to(self.wire_dtype)  # cast on the compute stream; the collective is ordered after it
            self.wire[b] = t
        self.works[b] = dist.all_reduce(t, group=self.pg, async_op=True)

    def bytes_on_wire(self):
        es = torch.empty((), dtype=self.wire_dtype or self.flat.dtype).element_size()
        return sum(n for _, n, _ in self.buckets) * es

    def hook(self, rt):
        """rt.unit_done for one backward pass (the pass that ends an accumulation window)."""
        side = getattr(rt, "side", None)

        def unit_done(unit):
            b = self.unit_bucket.get(unit)
            if b is None:
                return
            self.pending[b].discard(unit)
            if not self.pending[b]:
                self._issue(b, side)
        return unit_done

    def finish(self):
        """Issue the buckets not reported (none on the normal path), then wait for all of them; returns 1/world.
        With RCCL the waits are stream waits: the compute stream (clip / AdamW next) queues behind each bucket's
        collective, the host does not block.  bf16 wire buckets are cast back into the fp32 gradient here."""
        for b in range(len(self.buckets)):
            self._issue(b)
        if self.timing and torch.cuda.is_available() and self.flat.is_cuda:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        else:
            e0 = None
        for b, w in enumerate(self.works):
            w.wait()
            if self.wire[b] is not None:
                off, n, _ = self.buckets[b]
                self.flat[off:off + n].copy_(self.wire[b])
        if e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.exposed_ms.append((e0, e1))
        self.reset()
        return 1.0 / self.world

    def alone_ms(self, reps=3):
        """Time the window's all-reduces with nothing beside them (every bucket issued back to back, then waited):
        the denominator of the hidden-under-backward fraction.  Sums into the gradient: callers zero it after."""
        dev_ev = self.flat.is_cuda
        times = []
        for _ in range(reps):
            if dev_ev:
                torch.cuda.synchronize()
            dist.barrier(group=self.pg)
            t0 = torch.cuda.Event(enable_timing=True) if dev_ev else None
            if dev_ev:
                t0.record()
            for b in range(len(self.buckets)):
                self._issue(b)
            for b, w in enumerate(self.works):
                w.wait()
            if dev_ev:
                t1 = torch.cuda.Event(enable_timing=True)
                t1.record()
                torch.cuda.synchronize()
                times.append(t0.elapsed_time(t1))
            self.reset()
        return min(times) if times else None


def trainable(unet):
    """(master, grad, refresh) of what the step trains: the flat LoRA bucket (the reference's recipe), or every UNet
    parameter when unet.enable_full_grads() was called (BASELINE C3 / C4, build-only).  refresh(cast=True)."""
    if getattr(unet, "full", None) is not None:
        return unet.full.master, unet.full.grad, unet.refresh_full
    st = unet.lora
    return st.master, st.grad, st.refresh


def trainable_segments(unet):
    """[(offset, numel)] of the parameter tensors inside the flat trained buffer -- what the reference hands its
    optimizer (T:428-448: the peft lora_A / lora_B weights, or every UNet parameter in full-UNet mode); the 8-bit
    AdamW quantises each of them on its own (K.Adam8State)."""
    if getattr(unet, "full", None) is not None:
        fg = unet.full
        return [(fg.offsets[nm][0], p.numel()) for nm, p in zip(fg.names, fg.params)]
    st = unet.lora
    base = st.master.storage_offset()  # (element offsets: also defined for a meta-device state)
    segs = []
    for name in st.adapter_names():
        for t in st.adapter_views(st.master, name):
            segs.append((t.storage_offset() - base, t.numel()))
        if getattr(st, "dora", False):  # peft's lora_magnitude_vector: a parameter tensor of its own per module
            t = st.magnitude_view(st.master, name)
            segs.append((t.storage_offset() - base, t.numel()))
    return segs


def _work_copy(unet, master):
    """The flat bf16 working copy that refresh() casts the master into (the optimizer can write it directly)."""
    st = unet.full if getattr(unet, "full", None) is not None else unet.lora
    w = getattr(st, "work", None)
    ok = (w is not None and w.dtype == ELEM and w.numel() == master.numel() and w.is_contiguous()
          and w.data_ptr() % 16 == 0)
    return w if ok else None


class OptStep:
    """trainer.opt_step, the AdamW step count: a host integer, or -- with an amp.DeviceLossScaler, whose kernels
    advance it -- the state block's applied-step word, read back (a sync) only when somebody asks."""

    def __get__(self, tr, owner=None):
        if tr is None:
            return self
        sc = getattr(tr, "scaler", None)
        return sc.step if isinstance(sc, DeviceLossScaler) else tr.__dict__.get("opt_step", 0)

    def __set__(self, tr, value):
        sc = getattr(tr, "scaler", None)
        if isinstance(sc, DeviceLossScaler):
            sc.step = int(value)
        else:
            tr.__dict__["opt_step"] = int(value)


# the Prodigy arguments both trainers take (train.prodigy_* of a run config, --prodigy_* of the DreamBooth script)
PRODIGY_KEYS = ("prodigy_beta3", "prodigy_decouple", "prodigy_use_bias_correction", "prodigy_safeguard_warmup",
                "prodigy_d0", "prodigy_d_coef", "prodigy_growth_rate")


# the schedule arguments both trainers take (train.lr_* / train.max_train_steps of a run config, --lr_scheduler,
# --lr_warmup_steps, --max_train_steps, --lr_num_cycles, --lr_power of the DreamBooth script, DB:586-612)
LR_SCHEDULE_KEYS = ("lr_scheduler", "lr_warmup_steps", "max_train_steps", "lr_num_cycles", "lr_power")


def init_lr_schedule(tr, lr_scheduler="constant", lr_warmup_steps=0, max_train_steps=None, lr_num_cycles=1,
                     lr_power=1.0):
    """tr.lr_schedule: None for "constant" -- the optimizer step then runs the fixed-rate code unchanged -- else the
    lr_schedule.LrSchedule over tr.lr (which stays the base rate), stepped once per applied optimizer step
    (DB:1614-1621, 1962-1963), and tr.lr_word, the one-float device tensor the optimizer kernels read the step's lr
    from where the host cannot know it (amp.DeviceLossScaler: the applied-step count is on the device) or may not
    pass it (Prodigy's host-argument entry rejects the 0 every warm-up starts at)."""
    tr.lr_schedule = make_lr_schedule(lr_scheduler, tr.lr, lr_warmup_steps, max_train_steps, lr_num_cycles, lr_power)
    tr.lr_word = None
    if tr.lr_schedule is not None:
        tr.lr_word = torch.zeros(1, device=trainable(tr.unet)[0].device, dtype=torch.float32)


def sync_lr_word(tr):
    """After opt_step was set from outside (a checkpoint): the lr word holds the last applied step's lr again."""
    sched = getattr(tr, "lr_schedule", None)
    if sched is not None and getattr(tr, "lr_word", None) is not None:
        k = tr.opt_step
        tr.lr_word.fill_(sched.lr32(k - 1) if k >= 1 else 0.0)


class LastLr:
    """trainer.last_lr: the learning rate of the last applied optimizer step as the kernels saw it (float32), None
    before the first.  Without a schedule it is trainer.lr; with an amp.DeviceLossScaler it reads the device word --
    a sync, by request only, like the scaler's `.scale`."""

    def __get__(self, tr, owner=None):
        if tr is None:
            return self
        if tr.opt_step < 1:
            return None
        sched = getattr(tr, "lr_schedule", None)
        if sched is None:
            return float(tr.lr)
        if isinstance(getattr(tr, "scaler", None), DeviceLossScaler):
            return float(tr.lr_word.item())
        return sched.lr32(tr.opt_step - 1)


# the EMA arguments both trainers take (train.use_ema / train.ema_* of a run config, use_ema / ema_* of the DreamBooth
# namespace; diffusers' --use_ema and the EMAModel constructor)
EMA_ARG_KEYS = ("use_ema", "ema_decay", "ema_min_decay", "ema_update_after_step", "ema_use_warmup", "ema_inv_gamma",
                "ema_power")


def init_ema(tr, unet, use_ema=False, ema_decay=0.9999, ema_min_decay=0.0, ema_update_after_step=0,
             ema_use_warmup=False, ema_inv_gamma=1.0, ema_power=2 / 3):
    """tr.ema: None (the default: nothing is allocated or launched), or -- use_ema -- the ema.EMAModel over
    trainable(unet)'s flat master that the optimizer step updates once per call.  Every rank applies the same update to
    identical masters: no collective."""
    tr.ema = None
    if use_ema:
        from .ema import EMAModel
        tr.ema = EMAModel(unet, decay=ema_decay, min_decay=ema_min_decay, update_after_step=ema_update_after_step,
                          use_ema_warmup=ema_use_warmup, inv_gamma=ema_inv_gamma, power=ema_power)


def check_ema_live(tr, what):
    """Training on the averaged weights would silently corrupt the run: refuse while tr.ema's shadow is swapped in."""
    ema = getattr(tr, "ema", None)
    if ema is not None and ema.swapped:
        raise RuntimeError(f"{what} while the EMA weights are swapped in (EMAModel.copy_to / average_parameters): "
                           "restore() the live weights first")


def normalize_optimizer(name):
    """'adamw' or 'prodigy' (case-insensitive, the DreamBooth script's --optimizer, DB:622-627)."""
    opt = str(name).lower()
    if opt not in ("adamw", "prodigy"):
        raise ValueError(f"optimizer must be 'adamw' or 'prodigy', got {name!r}")
    return opt


def init_optimizer_state(tr, unet, optimizer="adamw", use_8bit_adam=False, prodigy_beta3=None, prodigy_decouple=True,
                         prodigy_use_bias_correction=False, prodigy_safeguard_warmup=False, prodigy_d0=1e-6,
                         prodigy_d_coef=1.0, prodigy_growth_rate=float("inf")):
    """The optimizer state of a trainer over trainable(unet)'s flat master: tr.optimizer, and either the AdamW state
    (tr.exp_avg / tr.exp_avg_sq, or tr.adam8 -- the blockwise 8-bit AdamW of bitsandbytes: uint8 codes + per-2048-block
    absmax, blocks restarting at every parameter tensor, 32-bit state under 4096 elements, K.Adam8State) or Prodigy's
    (tr.prodigy = K.ProdigyState, tr.prodigy_opts = the keyword arguments of K.prodigy_step; tr.exp_avg / exp_avg_sq
    then name its moments).  Prodigy has no 8-bit form: use_8bit_adam is ignored with a warning (DB:1486-1490)."""
    master, _, _ = trainable(unet)
    tr.optimizer = normalize_optimizer(optimizer)
    tr.prodigy = tr.prodigy_opts = None
    if tr.optimizer == "prodigy":
        if use_8bit_adam:
            import warnings
            warnings.warn("use_8bit_adam is ignored when optimizer is not set to 'AdamW' (it is 'prodigy')")
        tr.adam8 = None
        tr.prodigy = K.ProdigyState(master, d0=prodigy_d0)
        tr.prodigy_opts = dict(beta3=prodigy_beta3, decouple=bool(prodigy_decouple),
                               use_bias_correction=bool(prodigy_use_bias_correction),
                               safeguard_warmup=bool(prodigy_safeguard_warmup), d_coef=float(prodigy_d_coef),
                               growth_rate=float(prodigy_growth_rate))
        tr.exp_avg, tr.exp_avg_sq = tr.prodigy.exp_avg, tr.prodigy.exp_avg_sq
        return
    tr.adam8 = K.Adam8State(master.numel(), master.device, segments=trainable_segments(unet)) \
        if use_8bit_adam else None
    tr.exp_avg = None if use_8bit_adam else torch.zeros_like(master)
    tr.exp_avg_sq = None if use_8bit_adam else torch.zeros_like(master)


def lora_optimizer_step(tr):
    """accelerator.backward's sync step + clip_grad_norm_ + optimizer.step + zero_grad (T:857-861, DB:1953-1964) on
    the flat LoRA bucket of tr.unet: RCCL all-reduce -> global-norm clip coefficient -> fused AdamW (clip and 1/world
    folded into the gradient read) -> zero -> refresh the bf16 working copies.  tr carries exp_avg, exp_avg_sq,
    opt_step, clip_buf, lr, betas, adam_eps, wd, max_grad_norm, pg and, when the last backward of the window already
    issued the bucketed all-reduce (tr.sync_armed), the GradBuckets to finish.  fp16 training: tr.scaler is an
    amp.LossScaler (the norm is read back, one sync) or an amp.DeviceLossScaler (unscale / norm / clip -> step -> scale
    update, every decision -- inf-skip, step count, back-off and growth -- taken by the kernels on the scaler's state
    block: nothing is read back, and a skipped step still refreshes the unchanged working copies).
    tr.lr_schedule (None = the fixed rate tr.lr): the step runs at lr_schedule.lr(k), k = the steps applied before it.
    tr.ema (None = off; init_ema): ema.EMAModel.step() once per call, after the optimizer kernel -- and the opposite of
    the schedule's rule: the schedule counts APPLIED steps, so a step the loss scaler skips does not advance it, while
    the EMA counts accumulation windows, so the call is made on the host scaler's early return for a non-finite
    gradient and under the device scaler's skip as well, and the shadow then moves towards the unchanged master
    (diffusers' scripts call ema.step under accelerator.sync_gradients whether or not the scaler skipped)."""
    check_ema_live(tr, "optimizer_step")
    master, grad, refresh = trainable(tr.unet)
    if getattr(tr, "sync_armed", False):
        scale = tr.buckets.finish()
        tr.sync_armed = False
    else:
        scale = allreduce_grads(grad, tr.pg, getattr(tr, "allreduce_dtype", None))
    scaler = getattr(tr, "scaler", None)
    sched = getattr(tr, "lr_schedule", None)
    prodigy = getattr(tr, "prodigy", None)
    device_scaler = isinstance(scaler, DeviceLossScaler)
    # `src` = where the optimizer kernel takes the step's scalars from; `lr` = a float, or the device word
    if device_scaler:
        src = dict(amp_state=scaler.state)
        K.amp_unscale_clip(grad, tr.max_grad_norm, scaler.state, tr.betas, grad_scale=scale)
        # a schedule: the step's lr is evaluated on the device from the state's applied-step count (a skipped step
        # leaves the word as it was) and the kernels read it there; without one the host float goes in
        lr = tr.lr if sched is None else K.lr_schedule(sched, tr.lr_word, amp_state=scaler.state)
    else:
        if scaler is not None:
            # fp16 loss scaling (amp.LossScaler): the backward ran on loss * S, so unscale in the gradient read.  The
            # norm of the all-reduced gradient is read back -- the one sync per optimizer step, where GradScaler.step
            # syncs -- and every rank sees the same value.  Non-finite: skip the step whole (parameters, moments /
            # 8-bit state and opt_step untouched), drop the gradient, back the scale off (accelerate's inf-skip,
            # T:344-350).
            scale = scale / scaler.scale
        K.grad_clip_coef(grad, tr.max_grad_norm, grad_scale=scale, out=tr.clip_buf)
        if scaler is not None:
            found_inf = not math.isfinite(float(tr.clip_buf[0]))
            scaler.update(found_inf)
            if found_inf:
                K.zero_(grad)
                if getattr(tr, "ema", None) is not None:  # the EMA counts windows, not applied steps
                    tr.ema.step()
                return
        tr.opt_step += 1
        src = dict(step=tr.opt_step, grad_scale=scale, clip=tr.clip_buf)
        # a schedule (DB:1614-1621, stepped at DB:1962-1963): this step runs at lr(opt_step - 1) -- the host knows the
        # count here, so AdamW takes the value as the float it always took; Prodigy's host-argument entry rejects the
        # 0 a warm-up starts at, so its lr goes through the device word (one single-lane launch)
        if sched is None:
            lr = tr.lr
        elif prodigy is not None:
            lr = K.lr_schedule(sched, tr.lr_word, step=tr.opt_step)
        else:
            lr = sched.lr(tr.opt_step - 1)
    cast, zeroed = True, False
    if prodigy is not None:  # optimizer="prodigy": k, d and dlr stay on the device, so it takes no `step`
        src.pop("step", None)
        K.prodigy_step(master, grad, prodigy, lr, tr.betas, tr.adam_eps, tr.wd, **src, **tr.prodigy_opts)
    elif getattr(tr, "adam8", None) is not None:  # train.use_8bit_adam: bitsandbytes AdamW8bit (T:427-435)
        work = _work_copy(tr.unet, master)  # the step also writes the bf16 working copy (no separate cast pass)
        # with a per-tensor block table the step also zeroes the gradient it reads (the pads between tensors are
        # zero from allocation and no kernel writes them)
        zeroed = K.adamw8bit_step(master, grad, tr.adam8, lr, tr.betas, tr.adam_eps, tr.wd, out_bf16=work,
                                  zero_grad=True, **src)
        cast = work is None
    else:
        K.adamw_step(master, grad, tr.exp_avg, tr.exp_avg_sq, lr, tr.betas, tr.adam_eps, tr.wd, **src)
    if getattr(tr, "ema", None) is not None:  # once per call, skipped or not (the docstring)
        tr.ema.step()
    if device_scaler:
        K.amp_update(scaler.state, scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval)
    if not zeroed:
        K.zero_(grad)
    refresh(cast=cast)


class PSOTrainer:
    opt_step = OptStep()
    last_lr = LastLr()

    def __init__(self, unet, mode="turbo", num_steps=2, beta=50.0, clip_eps=0.1, lr=1e-5, betas=(0.9, 0.999),
                 weight_decay=1e-6, adam_eps=1e-8, max_grad_norm=1.0, gradient_accumulation_steps=1,
                 train_batch_size=1, num_reward=1, process_group=None, max_pass_images=16, ref_unet=None,
                 latent_dtype=torch.float32, allreduce_dtype=None, use_8bit_adam=False, overlap_sync=None,
                 bucket_mb=32.0, loss_scale=None, optimizer="adamw", prodigy_beta3=None, prodigy_decouple=True,
                 prodigy_use_bias_correction=False, prodigy_safeguard_warmup=False, prodigy_d0=1e-6,
                 prodigy_d_coef=1.0, prodigy_growth_rate=float("inf"), lr_scheduler="constant", lr_warmup_steps=0,
                 max_train_steps=None, lr_num_cycles=1, lr_power=1.0, fused_sampling=False, use_ema=False,
                 ema_decay=0.9999, ema_min_decay=0.0, ema_update_after_step=0, ema_use_warmup=False, ema_inv_gamma=1.0,
                 ema_power=2 / 3):
        self.unet = unet
        # fused_sampling: sample_pairs runs its forwards on merged weights W + s B A (unet.fuse_lora) and unfuses on
        # exit.  The loss never reads the sampling-time log-probs -- policy and reference are both recomputed at
        # train time -- so the training arithmetic is untouched.  Off (the default): nothing is built or launched.
        self.fused_sampling = bool(fused_sampling)
        if self.fused_sampling and getattr(unet, "lora", None) is None:
            raise ValueError("fused_sampling merges a LoRA adapter into the sampling weights: this UNet carries none")
        # loss_scale: None (no scaling), a float (initial scale), an amp.LossScaler or an amp.DeviceLossScaler (state
        # on the device, no sync in the optimizer step): dynamic loss scaling with inf-skip for fp16 training.
        # Active under the f16 library only -- bf16 has fp32's exponent range.
        self.scaler = make_scaler(loss_scale)
        if self.scaler is not None and ELEM != torch.float16:
            raise ValueError("loss_scale is for fp16 training (PSO_LIB=f16, libpso_amd_f16.so); the loaded library "
                             f"computes in {ELEM}")
        if mode not in ("turbo", "dmd"):
            raise ValueError(f"mode must be 'turbo' or 'dmd', got {mode!r}")
        # DMD2 with fp16 / bf16 latents: the reference's latent-dtype step / log-prob arithmetic (replay modes,
        # DP/distilled_inference_with_logprob.py:84-135); turbo upcasts to fp32 in the reference, so it stays fp32
        self.latent_dtype = latent_dtype if mode == "dmd" else torch.float32
        self.mode = MODE_TURBO if mode == "turbo" else pso_core.dmd_mode(self.latent_dtype)
        self.num_steps = num_steps
        self.T = num_steps - 1                       # the last (deterministic) step is never trained (T:218-221)
        self.beta, self.clip_eps = beta, clip_eps
        self.lr, self.betas, self.wd, self.adam_eps = lr, betas, weight_decay, adam_eps
        self.max_grad_norm = max_grad_norm
        self.gas = gradient_accumulation_steps
        self.gas_total = gradient_accumulation_steps * self.T  # Accelerator(gradient_accumulation_steps=gas*T) T:232
        self.P = train_batch_size
        self.m = num_reward
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        master, _, _ = trainable(unet)
        # optimizer state: fp32 AdamW moments, or -- train.use_8bit_adam, the reference default (T:427-435) -- the
        # blockwise 8-bit AdamW of bitsandbytes, or -- optimizer="prodigy" (lr around 1.0) -- Prodigy's
        init_optimizer_state(self, unet, optimizer=optimizer, use_8bit_adam=use_8bit_adam,
                             prodigy_beta3=prodigy_beta3, prodigy_decouple=prodigy_decouple,
                             prodigy_use_bias_correction=prodigy_use_bias_correction,
                             prodigy_safeguard_warmup=prodigy_safeguard_warmup, prodigy_d0=prodigy_d0,
                             prodigy_d_coef=prodigy_d_coef, prodigy_growth_rate=prodigy_growth_rate)
        # lr_scheduler / lr_warmup_steps / max_train_steps / lr_num_cycles / lr_power: diffusers' get_scheduler names
        # (DB:586-612); "constant" (the default) builds no schedule and the optimizer step is the fixed-rate one
        init_lr_schedule(self, lr_scheduler, lr_warmup_steps, max_train_steps, lr_num_cycles, lr_power)
        # use_ema (diffusers' --use_ema) / ema_*: the EMAModel arguments; off (the default) self.ema is None and nothing
        # is allocated or launched
        init_ema(self, unet, use_ema, ema_decay, ema_min_decay, ema_update_after_step, ema_use_warmup, ema_inv_gamma,
                 ema_power)
        self.opt_step = 0
        self.n_micro = 0
        self.clip_buf = torch.zeros(2, device=master.device, dtype=torch.float32)
        # full-UNet training (C3 / C4): the reference model is a frozen copy of the initial UNet (App. A #4), run as
        # its own forward instead of the adapter-free half of a paired pass
        self.ref_unet = ref_unet
        if getattr(unet, "full", None) is not None and ref_unet is None:
            raise ValueError("full-UNet training needs ref_unet (a frozen copy of the initial weights)")
        self.loss_hist = []
        # overlapped bucketed all-reduce on multi-GPU runs (GradBuckets); off inside hipGraph capture.  overlap_sync
        # forces it on (or off) whatever the world size: a world-1 RCCL group still runs every collective (tests)
        self.overlap_sync = (self.world > 1) if overlap_sync is None else bool(overlap_sync)
        if self.overlap_sync and not (dist.is_available() and dist.is_initialized()):
            raise ValueError("overlap_sync needs an initialised process group")
        # The default (None / torch.float32) is the reference's wire: DDP's fp32 all-reduce (T:228-233).  Opt-in:
        # torch.bfloat16 puts the gradient on a bf16 wire (fp32 accumulation and optimizer, GradBuckets); "auto" does
        # that for the full-UNet gradient only (C3 / C4: 10.3 GB fp32 per sync, 18 GB of ring traffic per rank at 8
        # ranks) and keeps the LoRA bucket fp32.  RCCL's ring re-rounds every partial sum on a bf16 wire, so its error
        # grows with the world size
        if isinstance(allreduce_dtype, str):
            if allreduce_dtype != "auto":
                raise ValueError(f"allreduce_dtype must be a torch dtype, None or 'auto', got {allreduce_dtype!r}")
            allreduce_dtype = torch.bfloat16 if getattr(unet, "full", None) is not None else None
        elif allreduce_dtype == torch.float32:
            allreduce_dtype = None
        self.allreduce_dtype = allreduce_dtype
        self.buckets = GradBuckets(unet, trainable(unet)[1], bucket_mb=bucket_mb, process_group=process_group,
                                   wire_dtype=allreduce_dtype) if self.overlap_sync else None
        self.sync_armed = False
        self.max_pass_images = max_pass_images  # images per batched UNet pass (HBM budget: ~5 GB saved each @1024^2)
        self.auto_step = True  # run the optimizer every gas*T micro-steps (tests may inspect raw grads)
        if self.mode == MODE_TURBO:
            self.sched = EulerAncestralDiscreteScheduler()
            self.sched.set_timesteps(num_steps)
            self.timesteps = self.sched.timesteps.clone()  # float32 [N]
        else:
            self.sched = LCMScheduler()
            ts, self.step_ratio = dmd_distill_timesteps(num_steps)
            self.timesteps = ts.float()
        dev = master.device
        self.timesteps_dev = self.timesteps.to(dev)
        # per-transition step coefficients [T, 8], host-computed once, device resident
        self.coef_dev = torch.stack([self.coef_for_step(j, 1)[0] for j in range(self.T)], 0).to(dev) \
            if self.T > 0 else torch.zeros(0, 8, device=dev)

    @classmethod
    def from_config(cls, unet, config, mode="turbo", num_reward=1, process_group=None, ref_unet=None,
                    latent_dtype=None, loss_scale=None):
        """Build from a reference run config (`config_sdxl_{turbo,dmd}_dpo.get_config()`): sample.num_steps,
        train.{beta, eps, learning_rate, adam_*, max_grad_norm, gradient_accumulation_steps, batch_size}.
        Both trainers require `distilled_train_steps == num_steps - 1` (turbo asserts it at T:221; DMD2 asserts
        `<=` at D:225 and the trajectory length `==` at D:719-720).
        latent_dtype (DMD2 only): None follows `config.mixed_precision` as the reference does -- its latents are
        weight_dtype (D:329-333; drawn in prompt_embeds.dtype, DP/sdxl_dmd_with_logprob.py:91-101), so its step /
        log-prob arithmetic runs in that dtype (DP/distilled_inference_with_logprob.py:84-135) -> the replay mode of
        that dtype; pass torch.float32 to train on the fp32 step math instead.  A value that disagrees with the
        config is honoured with a warning.
        loss_scale (f16 library only): the scaler to train with instead of the default host amp.LossScaler(), e.g.
        an amp.DeviceLossScaler.
        train.{lr_scheduler, lr_warmup_steps, max_train_steps, lr_num_cycles, lr_power} are read when present (the
        reference configs carry none: an absent lr_scheduler is "constant"), and so is train.fused_sampling
        (absent: False), and train.use_ema / train.ema_{decay, min_decay, update_after_step, use_warmup, inv_gamma,
        power} (absent: no EMA)."""
        tr = config.train
        if tr.distilled_train_steps != config.sample.num_steps - 1:
            raise AssertionError("train.distilled_train_steps must equal sample.num_steps - 1 "
                                 f"({tr.distilled_train_steps} vs {config.sample.num_steps - 1})")
        mp = getattr(config, "mixed_precision", "no")
        cfg_dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(mp, torch.float32)
        if latent_dtype is None:
            latent_dtype = cfg_dtype if mode == "dmd" else torch.float32
        elif mode == "dmd" and latent_dtype != cfg_dtype:
            import warnings
            warnings.warn(f"PSOTrainer.from_config: latent_dtype {latent_dtype} differs from the config's "
                          f"mixed_precision={mp!r} (reference latents: {cfg_dtype})")
        if ELEM == torch.float16:
            # the f16 library runs the reference's own recipe: fp16 UNet arithmetic, fp32 LoRA parameters, dynamic
            # loss scaling with inf-skip.  A config that asks for another precision belongs to the bf16 library.
            if mp != "fp16":
                raise ValueError(f"the f16 library (PSO_LIB=f16) trains mixed_precision='fp16' configs only, got "
                                 f"{mp!r}: unset PSO_LIB for the bf16 library")
            if loss_scale is None:
                loss_scale = LossScaler()
        return cls(unet, mode=mode, num_steps=config.sample.num_steps, beta=float(tr.beta), clip_eps=float(tr.eps),
                   lr=tr.learning_rate, betas=(tr.adam_beta1, tr.adam_beta2), weight_decay=tr.adam_weight_decay,
                   adam_eps=tr.adam_epsilon, max_grad_norm=tr.max_grad_norm,
                   gradient_accumulation_steps=tr.gradient_accumulation_steps, train_batch_size=tr.batch_size,
                   num_reward=num_reward, process_group=process_group, ref_unet=ref_unet, latent_dtype=latent_dtype,
                   use_8bit_adam=bool(getattr(tr, "use_8bit_adam", False)), loss_scale=loss_scale,
                   optimizer=getattr(tr, "optimizer", "adamw"),
                   fused_sampling=bool(getattr(tr, "fused_sampling", False)),
                   **{k: getattr(tr, k) for k in PRODIGY_KEYS + LR_SCHEDULE_KEYS + EMA_ARG_KEYS if hasattr(tr, k)})

    # ------------------------------------------------------------------------------------------------------------
    # coefficients of transition j (host float32 scalars, the reference's operation order)
    # ------------------------------------------------------------------------------------------------------------
    def coef_for_step(self, j, n):
        if self.mode == MODE_TURBO:
            t = self.timesteps[j].repeat(n)
            return pso_core.turbo_coef(self.sched.sigmas, self.sched.timesteps, t)
        t = self.timesteps[j].long().repeat(n)
        return pso_core.dmd_coef(self.sched.alphas_cumprod, t, t - self.step_ratio, latent_dtype=self.latent_dtype)

    # ------------------------------------------------------------------------------------------------------------
    # SAMPLING: B prompts -> 2 trajectories each (independent x_T, T:572-608) -> buffer rows
    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_pairs(self, enc, pooled, time_ids, h, generator=None, reward_fn=None, decode_fn=None):
        """enc [B,77,Dc] bf16, pooled [B,Dp], time_ids [B,6].  Returns a dict of NHWC buffer tensors.
        Both trajectories of a prompt are sampled in ONE UNet batch (image order 2b + k).
        fused_sampling: the forwards read merged weights; one merge per sampling phase that follows an optimizer step
        (fuse_lora's version check), none otherwise."""
        if not self.fused_sampling:
            return self._sample_pairs(enc, pooled, time_ids, h, generator, reward_fn, decode_fn)
        self.unet.fuse_lora()
        try:
            return self._sample_pairs(enc, pooled, time_ids, h, generator, reward_fn, decode_fn)
        finally:
            self.unet.unfuse_lora()

    def _sample_pairs(self, enc, pooled, time_ids, h, generator=None, reward_fn=None, decode_fn=None):
        dev = enc.device
        B = enc.shape[0]
        n_img = 2 * B
        N, T = self.num_steps, self.T
        enc2 = enc.repeat_interleave(2, 0).contiguous()
        pooled2 = pooled.repeat_interleave(2, 0).contiguous()
        tid2 = time_ids.repeat_interleave(2, 0).contiguous()
        shape = (n_img, h, h, 4)
        x = torch.randn(shape, device=dev, generator=generator, dtype=torch.float32)
        if self.mode == MODE_TURBO:
            x = x * float(self.sched.init_noise_sigma)
        elif self.latent_dtype != torch.float32:  # x_T drawn in the latent dtype (DP/sdxl_dmd_with_logprob.py:91-101)
            x = x.to(self.latent_dtype).float()
        member = torch.arange(n_img, device=dev) % 2
        xs, ins, lps = [x], [], []
        for i in range(N):
            t = self.timesteps_dev[i].repeat(n_img)
            if self.mode == MODE_TURBO:
                sig = float(self.sched.sigmas[i])
                model_in = K.cast_f32_bf16(x, scale=1.0 / math.sqrt(sig * sig + 1.0))  # DP/sdxl_turbo...:120-122
            else:
                model_in = K.cast_f32_bf16(x)
            eps, _ = self.unet.forward_nhwc(model_in, t, enc2, pooled2, tid2, save=False)
            if i < N - 1:
                coef = self.coef_for_step(i, n_img).to(dev)
                if self.mode == MODE_TURBO:
                    noise = torch.randn(shape, device=dev, generator=generator)
                    x, lp = K.step_logprob(self.mode, x, eps, coef, noise=noise)
                else:
                    # DMD2: each trajectory is its own sdxl_dmd_pipeline_with_logprob call (D:585-618) whose step
                    # re-noises with ONE (1,C,H,W) draw shared by that call's batch (DP/distilled_...:123-126): one
                    # draw per pair member k, shared by the prompts, never by the two members of a pair
                    noise = torch.randn((2,) + shape[1:], device=dev, generator=generator)
                    if self.latent_dtype != torch.float32:
                        noise = noise.to(self.latent_dtype).float()
                    x, lp = K.step_logprob(self.mode, x, eps, coef, noise=noise[member].contiguous())
                xs.append(x)
                ins.append(model_in)
                lps.append(lp)
            else:
                x_final = self._final_step(x, eps, n_img)
        x_stack = torch.stack(xs[:T + 1], 1)                    # [2B, T+1, h, h, 4]
        buf = dict(x=x_stack[:, :T].contiguous(), x_next=x_stack[:, 1:T + 1].contiguous(),
                   unet_in=torch.stack(ins, 1).contiguous(), lp=torch.stack(lps, 1), enc=enc2, pooled=pooled2,
                   tid=tid2)
        buf["x_final"] = x_final
        if reward_fn is not None:
            img = decode_fn(x_final) if decode_fn is not None else x_final
            buf["rewards"] = reward_fn(img).reshape(B, 2, -1).float()
        return buf

    def _final_step(self, x, eps, n):
        """Last sampler step (never trained): turbo sigma_to = 0 -> x + eps*(0 - sigma) (T:218-221); DMD2 returns
        x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t) (DP/sdxl_dmd_with_logprob.py:154-162)."""
        dev = x.device
        zero = torch.zeros((1,) + tuple(x.shape[1:]), device=dev)
        if self.mode == MODE_TURBO:
            c = self.coef_for_step(self.num_steps - 1, n)
        else:
            t = self.timesteps[-1].long().repeat(n)
            c = pso_core.dmd_coef(self.sched.alphas_cumprod, t, t)
            c[:, 2] = 1.0  # sqrt(abar_prev) -> 1: mean = x0
            c[:, 3] = 1.0
        xf, _ = K.step_logprob(self.mode, x, eps, c.to(dev), noise=zero, noise_shared=True)
        return xf

    # ------------------------------------------------------------------------------------------------------------
    # BUFFER shuffle (T:733-749): pair permutation + independent per-pair transition permutation, written out in
    # micro-step order so every micro-step reads contiguous [2P] slices.
    # ------------------------------------------------------------------------------------------------------------
    def shuffle(self, buf, generator=None):
        dev = buf["x"].device
        n_img = buf["x"].shape[0]
        Bp = n_img // 2
        T, P = self.T, self.P
        assert Bp % P == 0, "samples per epoch must be a multiple of train.batch_size (T:521-523)"
        perm = torch.randperm(Bp, device=dev, generator=generator)
        perms = torch.argsort(torch.rand((Bp, T), device=dev, generator=generator), dim=1)  # per-pair time perm
        nb = Bp // P
        img_idx, pair_img, tsel_i = shuffle_index(perm, perms, P)
        tt = self.timesteps_dev[tsel_i]
        out = SimpleNamespace(n_micro=nb * T, P=P)
        flat = lambda t: t.reshape((n_img * T,) + tuple(t.shape[2:]))
        out.x = K.gather_rows(flat(buf["x"]), img_idx)
        out.x_next = K.gather_rows(flat(buf["x_next"]), img_idx)
        out.unet_in = K.gather_rows(flat(buf["unet_in"]), img_idx)
        out.enc = K.gather_rows(buf["enc"], pair_img)
        out.pooled = K.gather_rows(buf["pooled"], pair_img)
        out.tid = K.gather_rows(buf["tid"], pair_img)
        out.t = tt.float().contiguous()
        out.coef = K.gather_rows(self.coef_dev, tsel_i)               # per-image step coefficients
        rw = buf["rewards"]                                       # [Bp, 2, m]
        out.rewards = rw[perm[(torch.arange(nb, device=dev)[:, None] * P + torch.arange(P, device=dev)[None])]]
        out.rewards = out.rewards.reshape(nb, 1, P, 2, -1).expand(nb, T, P, 2, rw.shape[-1]).reshape(-1, 2,
                                                                                                   rw.shape[-1])
        out.rewards = out.rewards.contiguous()
        return out

    def micro_batch(self, sb, s, count=1):
        """Micro-steps [s, s + count) of the shuffled stream (contiguous rows: 2P images per micro-step)."""
        n = 2 * self.P
        sl = slice(s * n, (s + count) * n)
        return SimpleNamespace(x=sb.x[sl], x_next=sb.x_next[sl], unet_in=sb.unet_in[sl], enc=sb.enc[sl],
                               pooled=sb.pooled[sl], tid=sb.tid[sl], t=sb.t[sl], coef=sb.coef[sl],
                               rewards=sb.rewards[s * self.P:(s + count) * self.P], count=count)

    # ------------------------------------------------------------------------------------------------------------
    # MICRO-STEP (T:773-861) -- no host synchronisation
    # ------------------------------------------------------------------------------------------------------------
    def micro_step(self, mb, generator=None):
        """One micro-step, or -- when mb holds `count` consecutive micro-steps of ONE accumulation window -- all of
        them in a single batched pass.  Inside a window the LoRA weights do not change (the optimizer steps only at
        the window end, T:857-861), so the batched pass produces the sum of the per-micro-step gradients: every
        pair's loss term keeps its weight 1 / (P * gas * T) (the per-micro-step mean over P pairs, divided by the
        accumulation count as accelerate does).  Larger batches keep the MFMA GEMMs fed (M = images * tokens)."""
        check_ema_live(self, "micro_step")
        count = getattr(mb, "count", 1)
        if self.n_micro // self.gas_total != (self.n_micro + count - 1) // self.gas_total:
            raise ValueError("a batched pass must not cross an optimizer step")
        P = self.P * count
        u = self.unet
        if self.ref_unet is not None:  # full-UNet training: policy pass + the frozen reference UNet's pass
            rs = _ref_stream() if _REF_STREAM and mb.unet_in.is_cuda else None
            if rs is not None:
                # the reference pass (different weights, same inputs, no saved state) on its own stream, beside the
                # policy pass: two grids of the small-M (6 images) GEMMs / attention fill the chip together
                main = torch.cuda.current_stream()
                rs.wait_stream(main)
                with torch.cuda.stream(rs), torch.no_grad():
                    eps_ref, _ = self.ref_unet.forward_nhwc(mb.unet_in, mb.t, mb.enc, mb.pooled, mb.tid, save=False)
                eps_pol, rt = u.forward_nhwc(mb.unet_in, mb.t, mb.enc, mb.pooled, mb.tid, save=True)
                main.wait_stream(rs)
                eps_ref.record_stream(main)
            else:
                eps_pol, rt = u.forward_nhwc(mb.unet_in, mb.t, mb.enc, mb.pooled, mb.tid, save=True)
                with torch.no_grad():
                    eps_ref, _ = self.ref_unet.forward_nhwc(mb.unet_in, mb.t, mb.enc, mb.pooled, mb.tid, save=False)
        else:
            u.enable_adapters()
            # policy (LoRA on, T:775-787) and reference (adapters disabled, T:790-805) eps of the same inputs in ONE pass
            eps_both, rt = u.forward_nhwc(mb.unet_in, mb.t, mb.enc, mb.pooled, mb.tid, save=True, paired_ref=True)
            n = mb.unet_in.shape[0]
            eps_pol, eps_ref = eps_both[:n], eps_both[n:]
        idx = None
        if self.mode == MODE_TURBO and self.m > 1:  # sample_compare draws a reward column per pair (T:405)
            idx = torch.randint(0, self.m, (P,), device=mb.x.device, generator=generator)
        pref = K.preference(mb.rewards, 0 if self.mode == MODE_TURBO else 1, reward_idx=idx)
        ws = K.pair_loss_ws(P, mb.x[0].numel(), mb.x.device)
        loss, lp = K.pair_loss_fwd(self.mode, mb.x, mb.x_next, eps_pol, eps_ref, mb.coef, pref, self.beta,
                                   self.clip_eps, ws)
        # accelerator.backward divides by gradient_accumulation_steps (accelerate accelerator.py:2840)
        if isinstance(self.scaler, DeviceLossScaler):  # the scale is read on the device (no host copy of it exists)
            deps = K.pair_loss_bwd(self.mode, mb.x, mb.x_next, eps_pol, mb.coef, pref, self.beta, self.clip_eps, ws,
                                   grad_out=self.scaler.scale_word, grad_scale=count / self.gas_total)
        else:
            deps = K.pair_loss_bwd(self.mode, mb.x, mb.x_next, eps_pol, mb.coef, pref, self.beta, self.clip_eps, ws,
                                   grad_scale=count / self.gas_total * self.loss_scale)
        if self.overlap_sync and self.auto_step and (self.n_micro + count) % self.gas_total == 0:
            rt.unit_done = self.buckets.hook(rt)  # the window's last backward: overlap the gradient all-reduce
            self.sync_armed = True
        u.backward_nhwc(deps, rt)
        self.loss_hist.append(loss)  # mean over the pass's pairs = mean of its micro-step losses
        self.n_micro += count
        if self.auto_step and self.n_micro % self.gas_total == 0:
            self.optimizer_step()
        return loss

    # ------------------------------------------------------------------------------------------------------------
    # SYNC (T:857-861): all-reduce (RCCL) -> clip -> AdamW -> zero -> refresh bf16 working copies
    # ------------------------------------------------------------------------------------------------------------
    def optimizer_step(self):
        lora_optimizer_step(self)

    @property
    def loss_scale(self):
        """The factor on the loss in backward: a power of two, constant within an accumulation window (it changes
        only in optimizer_step); 1.0 without a scaler.  With a DeviceLossScaler this reads the device (a sync)."""
        return 1.0 if self.scaler is None else self.scaler.scale

    _SB_TENSORS = ("x", "x_next", "unet_in", "enc", "pooled", "tid", "t", "coef", "rewards")

    def train_epoch_graph(self, sb, generator=None):
        """train_epoch as ONE hipGraph replay (torch.cuda.CUDAGraph over the HIP runtime): the epoch's micro-steps --
        paired UNet pass, fused loss, backward into the flat LoRA grad bucket -- are captured on the first call and
        replayed afterwards, so the ~7k kernel launches of an epoch cost one graph launch instead of one host call
        each.  The shuffled buffer is copied into the graph's static input buffers first; the optimizer step (with
        its all-reduce) runs eagerly after the replay.  Requires: the epoch is exactly one
        accumulation window starting at a window boundary, and the turbo sampler draws no reward column (m = 1);
        otherwise this is train_epoch."""
        if (sb.n_micro != self.gas_total or self.n_micro % self.gas_total or not self.auto_step
                or (self.mode == MODE_TURBO and self.m > 1)):
            return self.train_epoch(sb, generator)
        if getattr(self.unet, "full", None) is not None:
            # full-UNet training: the optimizer step rebuilds the kernel-layout weight caches as new tensors
            # (refresh_full -> prepare), which a captured graph would keep reading at their old addresses
            return self.train_epoch(sb, generator)
        key = tuple((k, tuple(getattr(sb, k).shape)) for k in self._SB_TENSORS)
        if not isinstance(self.scaler, DeviceLossScaler):
            # the loss scale is a host float baked into the captured loss backward: a change re-captures (rare).  A
            # device scaler's scale is read by the captured kernels: one capture serves every scale.
            key += (("loss_scale", self.loss_scale),)
        g = getattr(self, "_graph", None)
        if g is None or self._graph_key != key:
            self._graph = None
            # no collective inside the captured region: the step's all-reduce is eager.  Only the warm-up and the
            # capture run without the overlapped bucketed sync; eager epochs afterwards get it back (finally below).
            overlap0, self.overlap_sync = self.overlap_sync, False
            self._gsb = SimpleNamespace(n_micro=sb.n_micro, P=sb.P,
                                        **{k: getattr(sb, k).clone() for k in self._SB_TENSORS})
            _, st_grad, _ = trainable(self.unet)
            saved = st_grad.clone()
            self.auto_step = False
            n0, h0 = self.n_micro, len(self.loss_hist)
            try:
                self.train_epoch(self._gsb)  # eager warm-up of everything the capture will launch
                torch.cuda.synchronize()
                h1 = len(self.loss_hist)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self.train_epoch(self._gsb)
                self._gloss = self.loss_hist[h1:]
            finally:
                self.auto_step = True
                self.overlap_sync = overlap0
                self.n_micro = n0
                del self.loss_hist[h0:]
                st_grad.copy_(saved)
            self._graph, self._graph_key = g, key
        for k in self._SB_TENSORS:
            getattr(self._gsb, k).copy_(getattr(sb, k))
        self._graph.replay()
        self.loss_hist.extend(l.clone() for l in self._gloss)
        self.n_micro += sb.n_micro
        self.optimizer_step()

    def train_epoch(self, sb, generator=None):
        """One inner epoch over a shuffled buffer: every micro-step in order (T:755-861), batched per accumulation
        window up to `max_pass_images` images per UNet pass.  Python's cyclic garbage collector is paused for the
        epoch (PSO_GC_PAUSE=0 keeps it running): the ~3k kernel launches of a step allocate enough small objects to
        trigger collections in the middle of launch-bound stretches."""
        gc_on = _GC_PAUSE and gc.isenabled()
        if gc_on:
            gc.disable()
        try:
            self._train_epoch(sb, generator)
        finally:
            if gc_on:
                gc.enable()

    def _train_epoch(self, sb, generator=None):
        s = 0
        per_pass = max(1, self.max_pass_images // (2 * self.P))
        while s < sb.n_micro:
            left_in_window = self.gas_total - self.n_micro % self.gas_total
            c = min(per_pass, left_in_window, sb.n_micro - s)
            self.micro_step(self.micro_batch(sb, s, c), generator=generator)
            s += c
