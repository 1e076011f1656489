"""`generate_text` with the reference's contract (reference src/generation.py:6-52): run
model.generate over a loader and return `{index, task_type, generations}` records.  With args.with_scores and one beam each
record also carries "scores": the generations' sums of token log-probabilities (generate(return_logprobs=True))."""
from datetime import datetime


def _features(feats, device):
    """list of per-sample tensors (reference collator) or a kmbart.data.PackedFeatures (two copies, not B)"""
    return feats.to(device) if hasattr(feats, "packed") else [f.to(device) for f in feats]


def generate_text(model, gen_loader, tokenizer, args, device, logger=None, log_interval=1):
    n_steps = len(gen_loader)
    model.eval()
    t0 = datetime.now()
    records = []
    num_gen = args.num_gen
    with_scores = bool(getattr(args, "with_scores", False)) and args.num_beams == 1
    extra = {"return_logprobs": True} if with_scores else {}
    # the score processors only when asked for: an `args` without them calls generate() as before
    if getattr(args, "repetition_penalty", 1.0) != 1.0:
        extra["repetition_penalty"] = args.repetition_penalty
    if getattr(args, "no_repeat_ngram_size", 0) != 0:
        extra["no_repeat_ngram_size"] = args.no_repeat_ngram_size
    for i, batch in enumerate(gen_loader):
        out = model.generate(
            input_ids=batch["input_ids"].to(device),
            image_features=_features(batch["image_features"], device),
            attention_mask=batch["attention_mask"].to(device),
            num_beams=args.num_beams,
            num_return_sequences=num_gen,
            do_sample=getattr(args, "do_sample", False),
            top_p=getattr(args, "top_p", 1.0),
            top_k=getattr(args, "top_k", 0),
            early_stopping=True,
            **extra,
        )
        sums = None
        if with_scores:
            out, logprobs = out
            sums = logprobs.sum_logprobs.tolist()
        for j, index in enumerate(batch["index"]):
            texts = [tokenizer.decode(seq, skip_special_tokens=True) for seq in out[j * num_gen:(j + 1) * num_gen]]
            record = {"index": index, "task_type": batch["task_type"][j], "generations": texts}
            if sums is not None:
                record["scores"] = [float(x) for x in sums[j * num_gen:(j + 1) * num_gen]]
            records.append(record)
        if logger is not None and (i + 1) % log_interval == 0:
            eta = (n_steps - (i + 1)) / (i + 1) * (datetime.now() - t0)
            logger.info("Generating, Step [{}/{}], ETA: {}".format(i + 1, n_steps, str(eta)))
    return records
