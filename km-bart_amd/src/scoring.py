"""Perplexity filter with the contract of the reference's scripts/filter_reason.py:24-52: eval mode, one pass over the loader, a
sample's `dataset_index` is kept when the mean negative log-likelihood of its labels >= 0 -- the log of its perplexity -- is below
`args.pp_threshold`, and every step logs `Filtering, Step [i/N], ETA: ...`.

What differs is where the numbers come from: the reference takes the [B, T, V] logits of a forward without labels and picks the
label's log-softmax entry token by token on the host; here `model.score` returns the per-sample sums and counts from the device
(the head keeps softmax statistics only), and each batch costs ONE device-to-host copy."""
from datetime import datetime

import torch

from src.training import _features, _on


def sample_mean_nll(score):
    """[B] fp32: mean of -log p over a sample's valid labels = log(perplexity); NaN for a sample without one."""
    return score.nll / score.count.to(torch.float32)


def perplexity(score):
    """[B] fp32: exp(nll / count), the reference's `perplexity(pred, label)` for every sample of the batch at once."""
    return torch.exp(sample_mean_nll(score))


def perplexity_filter(model, loader, device, args, logger):
    kept = []
    n_steps = len(loader)
    model.eval()
    t0 = datetime.now()
    for i, batch in enumerate(loader):
        score = model.score(
            input_ids=batch["input_ids"].to(device), image_features=_features(batch["image_features"], device),
            attention_mask=_on(batch, "attention_mask", device), decoder_input_ids=_on(batch, "decoder_input_ids", device),
            decoder_attention_mask=_on(batch, "decoder_attention_mask", device), labels=batch["labels"].to(device))
        log_pp = sample_mean_nll(score).cpu().tolist()   # the batch's one copy to the host (it also waits for the batch)
        for j, v in enumerate(log_pp):
            if v < args.pp_threshold:   # NaN (no valid label) compares false: never kept
                kept.append(batch["dataset_index"][j])
        if logger is not None:
            eta = (n_steps - (i + 1)) / (i + 1) * (datetime.now() - t0)
            logger.info("Filtering, Step [{}/{}], ETA: {}".format(i + 1, n_steps, str(eta)))
    return kept
