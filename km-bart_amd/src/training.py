"""Training loop with the reference's `fine_tune` contract (reference src/training.py:96-171):
forward -> zero_grad -> (scaled) backward -> optimizer step, per-step log line
`Epoch [e/E], Step [i/N], Loss: x.xxxx, ETA: ...`, optional TensorBoard scalars and a callback.

One deliberate difference in timing, none in content: the reference reads `loss.item()` right after forward
(training.py:134), which stalls the host until the GPU has drained and leaves the GPU idle while the host enqueues
the next ~600 launches.  Here step i's loss is read AFTER step i+1 has been enqueued (the last one after the loop), so
log lines / TensorBoard points / the returned epoch mean carry the same values, one step later.  A `callback` gets
called in step order as in the reference; it forces the pending loss to be read first.

Gradient accumulation (`args.accumulation_steps = N > 1`, not in the reference): the batches of the loader are micro-batches, taken in
groups of N (the last group of an epoch may be shorter).  `optimizer.zero_grad()` runs on a group's first micro-batch, every
micro-batch runs `(loss / N).backward()` -- the mean over the group of the micro-batches' mean losses; a short last group is still
divided by N -- and `optimizer.step()` runs on the group's last one.  Under the data-parallel wrapper the other micro-batches run
inside its `no_sync()`: one gradient exchange per optimizer step.  Log lines, the callback and the returned epoch mean stay per
micro-batch and carry the unscaled loss; the gradient-norm line appears on optimizer steps only."""
import contextlib
import sys
from datetime import datetime

import torch


def _on(batch, key, device):
    return batch[key].to(device) if key in batch and batch[key] is not None else None


def _allow_overlap(optimizer, ok):
    """These loops run `loss.backward()` and `optimizer.step()` back to back with nothing touching the gradients in
    between: kmbart.optim.AdamW may then step each gradient bucket beside the rest of backward (see its __init__)."""
    if hasattr(optimizer, "allow_overlap"):
        optimizer.allow_overlap(ok)


def _step_record(optimizer):
    """An optimizer that clips / guards its own step (kmbart.optim.AdamW(max_grad_norm=..., skip_nonfinite=...)): a device copy of
    the step's record, taken in stream order right behind `step()` -- no synchronisation; None for any other optimizer."""
    return optimizer.step_record() if getattr(optimizer, "guarded", False) else None


def _norm_line(record, logger, epoch, args, j, n_steps):
    """ONE additional line of the per-interval log: the gradient norm of step j and the steps skipped so far (read where the
    loss is read, one step behind the enqueue)."""
    if record is not None:
        st = record.read()
        logger.info("Epoch [{}/{}], Step [{}/{}], Grad norm: {:.4f}, Skipped steps: {}".format(
            epoch + 1, args.epochs, j + 1, n_steps, st["norm"], st["skipped"]))


def _attach(model, optimizer, ok):
    """Data-parallel wrapper: chain each gradient piece's optimizer update behind its all-reduce (kmbart.parallel)."""
    if ok and hasattr(model, "attach_optimizer"):
        model.attach_optimizer(optimizer)


def _accumulation_steps(args):
    n = getattr(args, "accumulation_steps", 1)
    n = 1 if n is None else int(n)
    if n < 1:
        raise ValueError("accumulation_steps must be >= 1, got %d" % n)
    return n


def _micro_step(i, n_steps, n_accum):
    """(first, last) of micro-batch i of a loader of n_steps batches taken in groups of n_accum: zero_grad runs on a group's first
    micro-batch, the optimizer steps on its last -- which is also the loader's last batch when the final group is short."""
    return i % n_accum == 0, (i % n_accum == n_accum - 1 or i == n_steps - 1)


def _accumulate(model, on):
    """Switches the engine's gradient accumulation (model.accumulate_gradients, through a data-parallel wrapper's .module)."""
    target = model if hasattr(model, "accumulate_gradients") else getattr(model, "module", None)
    if not hasattr(target, "accumulate_gradients"):
        raise RuntimeError("accumulation_steps > 1 needs a model with accumulate_gradients(): a backward of this engine overwrites "
                           "the gradients, nothing outside it can add them up")
    target.accumulate_gradients(on)


def _sync_scope(model, sync):
    """The data-parallel wrapper's no_sync() around a micro-batch that is not its group's last; nothing otherwise."""
    if not sync and hasattr(model, "no_sync"):
        return model.no_sync()
    return contextlib.nullcontext()


def _release(model, optimizer, accumulating=False):
    """The fusions above hold only inside these loops: afterwards `optimizer.step()` is a plain step and `loss.backward()` a plain
    backward that OVERWRITES the gradients again (clip_grad_norm_, a diagnostic backward; accumulation the loop switched on is
    switched off here -- a loop of the caller's own asks for it with model.accumulate_gradients())."""
    failing = sys.exc_info()[0] is not None   # (called from the loops' `finally`: an error of the loop's is on its way out)
    _allow_overlap(optimizer, False)
    if hasattr(model, "detach_optimizer"):
        model.detach_optimizer()
    if accumulating:
        try:
            _accumulate(model, False)
        except Exception:
            if not failing:   # (else the loop's error is the one to report: it may have left a forward without its backward)
                raise


def _features(feats, device):
    """list of per-sample tensors (reference collator) or a kmbart.data.PackedFeatures"""
    return feats.to(device) if hasattr(feats, "packed") else [f.to(device) for f in feats]


def fine_tune(epoch, model, train_loader, optimizer, device, args, logger=None, callback=None, log_interval=1,
              tb_writer=None, tb_interval=1, scaler=None):
    n_accum = _accumulation_steps(args)
    try:
        if n_accum > 1:
            _accumulate(model, True)
        return _fine_tune(epoch, model, train_loader, optimizer, device, args, logger, callback, log_interval, tb_writer,
                          tb_interval, scaler, n_accum)
    finally:
        _release(model, optimizer, n_accum > 1)


def _fine_tune(epoch, model, train_loader, optimizer, device, args, logger, callback, log_interval, tb_writer, tb_interval,
               scaler, n_accum=1):
    n_steps = len(train_loader)
    model.train()
    t0 = datetime.now()
    use_amp = bool(getattr(args, "amp", False))
    _allow_overlap(optimizer, not (use_amp and scaler is not None))
    _attach(model, optimizer, not (use_amp and scaler is not None))
    pending = None
    state = {"sum": 0.0}

    def report(item):
        if item is None:
            return
        j, dev_loss, _, record = item
        loss_value = dev_loss.item()
        state["sum"] += loss_value
        if logger is not None and j % log_interval == 0:
            eta = (n_steps - (j + 1)) / (j + 1) * (datetime.now() - t0)
            logger.info("Epoch [{}/{}], Step [{}/{}], Loss: {:.4f}, ETA: {}".format(
                epoch + 1, args.epochs, j + 1, n_steps, loss_value, str(eta)))
            _norm_line(record, logger, epoch, args, j, n_steps)
        if tb_writer is not None and j % tb_interval == 0:
            tb_writer.add_scalars("loss/step", {"loss": loss_value}, epoch * n_steps + j + 1)

    for i, batch in enumerate(train_loader):
        # the engine computes in bf16 with fp32 accumulation regardless of `amp`; autocast is kept so
        # that torch ops a caller adds around the model behave as in the reference
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=use_amp and torch.cuda.is_available()):
            outputs = model.forward(
                input_ids=batch["input_ids"].to(device),
                image_features=_features(batch["image_features"], device),
                attention_mask=batch["attention_mask"].to(device),
                decoder_input_ids=_on(batch, "decoder_input_ids", device),
                decoder_attention_mask=_on(batch, "decoder_attention_mask", device),
                labels=batch["labels"].to(device),
                answer_ids=_on(batch, "answer_ids", device),
                answer_attention_mask=_on(batch, "answer_attention_mask", device),
            )
            loss = outputs[0]
        first, last = _micro_step(i, n_steps, n_accum)
        if first:
            optimizer.zero_grad()
        micro_loss = loss if n_accum == 1 else loss / n_accum
        with _sync_scope(model, last):
            if use_amp and scaler is not None:
                scaler.scale(micro_loss).backward()
            else:
                micro_loss.backward()
        if last:
            if use_amp and scaler is not None:
                scaler.step(optimizer)
                scaler.update()
            else:
                optimizer.step()
        report(pending)                       # step i-1, while step i runs on the GPU
        pending = (i, loss.detach(), None, _step_record(optimizer) if last else None)
        if callback is not None:
            report(pending)
            pending = None
            callback(step=i, epoch=epoch, model=model, train_loader=train_loader, optimizer=optimizer, args=args,
                     logger=logger)
    report(pending)
    loss_sum = state["sum"]
    if tb_writer is not None:
        tb_writer.add_scalars("loss/epoch", {"train": loss_sum / max(n_steps, 1)}, epoch + 1)
    return loss_sum / max(n_steps, 1)


def pretrain(epoch, model, train_loader, optimizer, device, args, logger=None, callback=None, log_interval=1,
             tb_writer=None, tb_interval=1, scaler=None):
    """Multi-task pre-training loop with the reference's contract (reference src/training.py:9-93): the model
    returns a dict of losses as outputs[0]; `loss` drives backward, the others are logged."""
    n_accum = _accumulation_steps(args)
    try:
        if n_accum > 1:
            _accumulate(model, True)
        return _pretrain(epoch, model, train_loader, optimizer, device, args, logger, callback, log_interval, tb_writer,
                         tb_interval, scaler, n_accum)
    finally:
        _release(model, optimizer, n_accum > 1)


def _pretrain(epoch, model, train_loader, optimizer, device, args, logger, callback, log_interval, tb_writer, tb_interval,
              scaler, n_accum=1):
    n_steps = len(train_loader)
    model.train()
    t0 = datetime.now()
    use_amp = bool(getattr(args, "amp", False))
    _allow_overlap(optimizer, not (use_amp and scaler is not None))
    _attach(model, optimizer, not (use_amp and scaler is not None))
    pending = None
    state = {"sum": 0.0}

    def report(item):
        if item is None:
            return
        j, dev_loss, parts, record = item
        loss_value = dev_loss.item()
        state["sum"] += loss_value
        if logger is not None and j % log_interval == 0:
            eta = (n_steps - (j + 1)) / (j + 1) * (datetime.now() - t0)
            logger.info("Epoch [{}/{}], Step [{}/{}], Loss: {:.4f}, ETA: {}".format(
                epoch + 1, args.epochs, j + 1, n_steps, loss_value, str(eta)))
            _norm_line(record, logger, epoch, args, j, n_steps)
        if tb_writer is not None and j % tb_interval == 0:
            step = epoch * n_steps + j + 1
            tb_writer.add_scalars("loss/step", {"total loss": loss_value}, step)
            for name, value in parts.items():
                tb_writer.add_scalars("loss/step", {name.replace("_", " "): value.item()}, step)

    for i, batch in enumerate(train_loader):
        def opt(key):
            return batch[key].to(device) if key in batch and batch[key] is not None else None

        def opt_list(key):
            return [t.to(device) for t in batch[key]] if key in batch else None

        outputs = model.forward(
            input_ids=batch["input_ids"].to(device),
            image_features=_features(batch["image_features"], device),
            attention_mask=batch["attention_mask"].to(device),
            decoder_input_ids=opt("decoder_input_ids"),
            decoder_attention_mask=opt("decoder_attention_mask"),
            labels=opt("labels"),
            mrm_labels=opt_list("mrm_labels"),
            mrm_mask=opt("mrm_mask"),
            attribute_labels=opt_list("attribute_labels"),
            attribute_mask=opt("attribute_mask"),
            relation_labels=batch.get("relation_labels"),
        )
        losses = outputs[0]
        loss = losses["loss"]
        first, last = _micro_step(i, n_steps, n_accum)
        if first:
            optimizer.zero_grad()
        micro_loss = loss if n_accum == 1 else loss / n_accum
        with _sync_scope(model, last):
            if use_amp and scaler is not None:
                scaler.scale(micro_loss).backward()
            else:
                micro_loss.backward()
        if last:
            if use_amp and scaler is not None:
                scaler.step(optimizer)
                scaler.update()
            else:
                optimizer.step()
        report(pending)
        pending = (i, loss.detach(), {k: v.detach() for k, v in losses.items() if k != "loss"},
                   _step_record(optimizer) if last else None)
        if callback is not None:
            report(pending)
            pending = None
            callback(step=i, epoch=epoch, model=model, train_loader=train_loader, optimizer=optimizer, args=args,
                     logger=logger)
    report(pending)
    loss_sum = state["sum"]
    if tb_writer is not None:
        tb_writer.add_scalars("loss/epoch", {"train": loss_sum / max(n_steps, 1)}, epoch + 1)
    return loss_sum / max(n_steps, 1)


def self_critical_fine_tune(epoch, model, train_loader, optimizer, device, args, reward, logger=None, callback=None,
                            log_interval=1, tb_writer=None, tb_interval=1, baseline="greedy", sample_kwargs=None, samples_per_input=1):
    """`fine_tune` with the self-critical loss in place of the cross-entropy: per batch `self_critical_step` with
    `reward.for_batch(batch)` (src.rewards.CiderReward: the reward is computed on the device), then zero_grad -> backward ->
    optimizer step in fine_tune's order, with its accumulation and its data-parallel scopes.  The log line is fine_tune's plus the
    batch's mean reward and mean advantage:
    `Epoch [e/E], Step [i/N], Loss: x.xxxx, Reward: x.xxxx, Advantage: x.xxxx, ETA: ...`.
    Values are read back only where fine_tune reads its loss: step i's after step i + 1 has been enqueued.  Returns the epoch's
    mean loss.  baseline: "greedy", "mean" (samples_per_input >= 2) or None; sample_kwargs goes to self_critical_step (max_length, ...);
    samples_per_input = G > 1: G samples per input, `reward.for_batch(batch, repeats=G)`, one grouped forward (self_critical_step)."""
    n_accum = _accumulation_steps(args)
    try:
        if n_accum > 1:
            _accumulate(model, True)
        return _self_critical_fine_tune(epoch, model, train_loader, optimizer, device, args, reward, logger, callback,
                                        log_interval, tb_writer, tb_interval, baseline, sample_kwargs, n_accum, samples_per_input)
    finally:
        _release(model, optimizer, n_accum > 1)


def _self_critical_fine_tune(epoch, model, train_loader, optimizer, device, args, reward, logger, callback, log_interval,
                             tb_writer, tb_interval, baseline, sample_kwargs, n_accum=1, samples_per_input=1):
    n_steps = len(train_loader)
    model.train()
    t0 = datetime.now()
    _allow_overlap(optimizer, True)
    _attach(model, optimizer, True)
    pending = None
    state = {"sum": 0.0}

    def report(item):
        if item is None:
            return
        j, dev_values, _, record = item
        loss_value, reward_value, advantage_value = dev_values.tolist()   # one read for the three
        state["sum"] += loss_value
        if logger is not None and j % log_interval == 0:
            eta = (n_steps - (j + 1)) / (j + 1) * (datetime.now() - t0)
            logger.info("Epoch [{}/{}], Step [{}/{}], Loss: {:.4f}, Reward: {:.4f}, Advantage: {:.4f}, ETA: {}".format(
                epoch + 1, args.epochs, j + 1, n_steps, loss_value, reward_value, advantage_value, str(eta)))
            _norm_line(record, logger, epoch, args, j, n_steps)
        if tb_writer is not None and j % tb_interval == 0:
            tb_writer.add_scalars("loss/step", {"loss": loss_value, "reward": reward_value, "advantage": advantage_value},
                                  epoch * n_steps + j + 1)

    for i, batch in enumerate(train_loader):
        if samples_per_input > 1:
            loss, info = self_critical_step(model, batch, reward.for_batch(batch, repeats=samples_per_input), device, baseline=baseline,
                                            sample_kwargs=sample_kwargs, samples_per_input=samples_per_input)
        else:
            loss, info = self_critical_step(model, batch, reward.for_batch(batch), device, baseline=baseline,
                                            sample_kwargs=sample_kwargs)
        first, last = _micro_step(i, n_steps, n_accum)
        if first:
            optimizer.zero_grad()
        micro_loss = loss if n_accum == 1 else loss / n_accum
        with _sync_scope(model, last):
            micro_loss.backward()
        if last:
            optimizer.step()
        report(pending)                       # step i-1, while step i runs on the GPU
        values = torch.stack([loss.detach().float().reshape(()), info["rewards"].mean(), info["advantages"].mean()])
        pending = (i, values, None, _step_record(optimizer) if last else None)
        if callback is not None:
            report(pending)
            pending = None
            callback(step=i, epoch=epoch, model=model, train_loader=train_loader, optimizer=optimizer, args=args,
                     logger=logger)
    report(pending)
    loss_sum = state["sum"]
    if tb_writer is not None:
        tb_writer.add_scalars("loss/epoch", {"train": loss_sum / max(n_steps, 1)}, epoch + 1)
    return loss_sum / max(n_steps, 1)


def leave_one_out_baseline(rewards, samples_per_input):
    """The multi-sample self-critical baseline: rewards [B * G] in groups of G consecutive rows (the row order of
    generate(num_return_sequences=G)); b_i = (sum of the group's rewards - r_i) / (G - 1), the mean reward of the input's OTHER samples.
    Needs G >= 2 (ValueError).  The advantages r - b of a group sum to zero.  Device ops only."""
    G = int(samples_per_input)
    if G < 2:
        raise ValueError("the 'mean' (leave-one-out) baseline needs samples_per_input >= 2, got %d" % G)
    if rewards.dim() != 1 or rewards.shape[0] % G != 0:
        raise ValueError("rewards must be [batch * samples_per_input], got %s with samples_per_input = %d" % (tuple(rewards.shape), G))
    r = rewards.view(-1, G)
    return ((r.sum(dim=1, keepdim=True) - r) / (G - 1)).reshape(-1)


def self_critical_step(model, batch, reward_fn, device, baseline="greedy", sample_kwargs=None, samples_per_input=1):
    """One REINFORCE / self-critical loss (Rennie et al. 2017) on `batch` (input_ids, image_features, attention_mask):
    under no_grad one `generate(do_sample=True, num_beams=1, top_k=0, top_p=1.0, ...)` draws a sequence per input from the model's
    full distribution; `reward_fn(ids) -> float32 [B]` scores it (any callable; src.rewards.CiderReward.for_batch(batch) is a CIDEr-D
    computed on the device); the advantage is A = reward(sample) - baseline with baseline = the reward of one greedy `generate(num_beams=1)` ("greedy"), zero (None) or a
    given [B] tensor.  Then ONE teacher-forced forward on the samples (src/model/utils.py::labels_from_generated) with
    `loss_weights = A / B, loss_reduction="sum"`:  loss = -(1 / B) sum_b A_b log p(y_b | x_b), whose gradient is the policy gradient.
    Returns (loss, info); the caller runs `loss.backward()` and steps its optimizer.  info: `sample_ids`, `advantages`, `rewards`
    and `baseline` as device tensors (and `greedy_ids` with the greedy baseline); nothing here reads a value back.
    `sample_kwargs` goes to both generate calls (max_length, min_length, ...); its `pad_to_multiple_of` (optional) goes to
    labels_from_generated instead.  Sampling is unfiltered on purpose: the forward's gradient is that of the full log-softmax, which is
    the sampler's log-probability only without top-k / top-p filtering.
    `samples_per_input` = G > 1: the sampling generate draws G sequences per input (num_return_sequences=G: rows i G .. i G + G - 1 belong
    to input i), `reward_fn` scores the [B * G] rows (CiderReward.for_batch(batch, repeats=G)), and the ONE forward is grouped --
    `targets_per_input=G` on the B inputs, the encoder side run once -- with `loss_weights = A / (B G)`.  baseline "mean" (G >= 2 only): the
    leave-one-out mean of the input's other samples (leave_one_out_baseline), no greedy pass; "greedy": the one greedy sequence of an input,
    scored once per sample row, i.e. its reward broadcast over the input's G samples; a tensor: [B * G].  info's tensors have B * G rows."""
    from src.model.utils import labels_from_generated

    kw = dict(sample_kwargs or {})
    pad_to = kw.pop("pad_to_multiple_of", None)
    for fixed in ("do_sample", "num_beams", "top_k", "top_p", "num_return_sequences"):
        if fixed in kw:
            raise ValueError("self_critical_step fixes %s itself (unfiltered one-beam sampling)" % fixed)
    G = int(samples_per_input)
    if G < 1:
        raise ValueError("samples_per_input must be at least 1, got %d" % G)
    if baseline == "mean" and G < 2:
        raise ValueError("the 'mean' (leave-one-out) baseline needs samples_per_input >= 2, got %d" % G)
    skw = dict(kw, num_return_sequences=G) if G > 1 else kw
    input_ids = batch["input_ids"].to(device)
    image_features = _features(batch["image_features"], device)
    attention_mask = batch["attention_mask"].to(device)
    info = {}
    with torch.no_grad():
        sample_ids = model.generate(input_ids=input_ids, image_features=image_features, attention_mask=attention_mask,
                                    do_sample=True, num_beams=1, top_k=0, top_p=1.0, **skw)
        rewards = reward_fn(sample_ids).to(device=device, dtype=torch.float32)
        if baseline is None:
            base = torch.zeros_like(rewards)
        elif isinstance(baseline, str):
            if baseline == "mean":
                base = leave_one_out_baseline(rewards, G)
            elif baseline == "greedy":
                greedy_ids = model.generate(input_ids=input_ids, image_features=image_features, attention_mask=attention_mask,
                                            do_sample=False, num_beams=1, **kw)
                # (G > 1: reward_fn scores B * G rows, row i against input i // G: the greedy sequence once per sample row)
                base = reward_fn(greedy_ids.repeat_interleave(G, dim=0) if G > 1 else greedy_ids).to(device=device, dtype=torch.float32)
                info["greedy_ids"] = greedy_ids
            else:
                raise ValueError("baseline must be 'greedy', 'mean', None or a [B] tensor, got %r" % (baseline,))
        else:
            base = baseline.to(device=device, dtype=torch.float32)
        advantages = rewards - base
    cfg = getattr(model, "module", model).config
    pad_id = kw.get("pad_token_id", cfg.pad_token_id)
    eos_id = kw.get("eos_token_id", cfg.eos_token_id)
    dec_in, dec_mask, labels = labels_from_generated(sample_ids, pad_id, eos_id, pad_to_multiple_of=pad_to)
    B = sample_ids.shape[0]
    outputs = model.forward(input_ids=input_ids, image_features=image_features, attention_mask=attention_mask,
                            decoder_input_ids=dec_in, decoder_attention_mask=dec_mask, labels=labels,
                            loss_weights=advantages / B, loss_reduction="sum", **({"targets_per_input": G} if G > 1 else {}))
    info.update(sample_ids=sample_ids, advantages=advantages, rewards=rewards, baseline=base)
    return outputs[0], info
