"""`sample_sentence` with the reference's contract (reference src/model/utils.py:6-58): nucleus-sample one sequence per input
and return it with the sum of its tokens' log-probabilities; `labels_from_generated` turns generated ids into the teacher-forced
batch whose weighted cross-entropy differentiates those log-probabilities (src/training.py::self_critical_step)."""
import torch


def sample_sentence(model, input_ids, image_features, attention_mask, tokenizer, top_k=50, top_p=1.0, max_length=20):
    """Samples from BOS until every row has drawn EOS or max_length is reached, each token from softmax(top-k / top-p filtered
    logits) at temperature 1 with no min_length ban and no score processors.  Returns (decoder_input_ids [B, L],
    sum_logprobs [B, 1]): per row the sum of log_softmax(filtered logits)[token] over its tokens up to and including EOS
    (finished rows are fed pad tokens and add nothing), not length-normalised.
    One generate(do_sample=True, num_beams=1, return_logprobs=True) call: the KV-cached decode loop with the device sampler
    instead of the reference's uncached forward per step.  The one difference from the reference: the values are returned
    without an autograd graph (generate runs under no_grad), so they can weigh or rank samples but not be differentiated here;
    src/training.py::self_critical_step differentiates them through `forward(labels=..., loss_weights=..., loss_reduction="sum")`."""
    ids, logprobs = model.generate(
        input_ids=input_ids, image_features=image_features, attention_mask=attention_mask, do_sample=True, num_beams=1,
        return_logprobs=True, top_k=top_k, top_p=top_p, max_length=max_length, temperature=1.0, min_length=0,
        num_return_sequences=1, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None,
        decoder_start_token_id=tokenizer.bos_token_id, pad_token_id=tokenizer.pad_token_id, eos_token_id=tokenizer.eos_token_id)
    return ids, logprobs.sum_logprobs.unsqueeze(1)


def labels_from_generated(ids, pad_token_id, eos_token_id, pad_to_multiple_of=None):
    """The teacher-forced batch of ids [B, L] as `generate` returns them (start token first): (decoder_input_ids [B, T],
    decoder_attention_mask [B, T], labels [B, T]) with decoder_input_ids = ids[:, :-1] and labels = ids[:, 1:], T = L - 1.
    A row's first EOS is kept as a label and everything behind it is -100 -- the `sent_lengths` rule of the reference's
    sample_sentence (src/model/utils.py:42-54), so the sum of a row's token log-probabilities over its valid labels is that row's
    `sum_logprobs`; a row without EOS keeps all its labels.  The mask is 1 where the label is valid (attention is causal: the
    positions behind cannot reach the ones before).  `pad_to_multiple_of` pads T up to a multiple (pad ids, mask 0, labels -100),
    e.g. so that B * T is a whole number of 256-row tiles, the fused head's condition.  Device tensor ops only: nothing
    synchronises."""
    dec_in = ids[:, :-1]
    nxt = ids[:, 1:]
    is_eos = (nxt == eos_token_id).long()
    eos_before = torch.cumsum(is_eos, dim=1) - is_eos   # the EOS tokens strictly in front of each position
    valid = eos_before == 0
    labels = torch.where(valid, nxt, torch.full_like(nxt, -100))
    mask = valid.long()
    if pad_to_multiple_of:
        m = int(pad_to_multiple_of)
        extra = (-dec_in.shape[1]) % m
        if extra:
            B = ids.shape[0]
            dec_in = torch.cat([dec_in, dec_in.new_full((B, extra), pad_token_id)], dim=1)
            labels = torch.cat([labels, labels.new_full((B, extra), -100)], dim=1)
            mask = torch.cat([mask, mask.new_zeros((B, extra))], dim=1)
    return dec_in.contiguous(), mask, labels
