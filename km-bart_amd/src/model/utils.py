"""`sample_sentence` with the reference's contract (reference src/model/utils.py:6-58): nucleus-sample one sequence per input
and return it with the sum of its tokens' log-probabilities."""


def sample_sentence(model, input_ids, image_features, attention_mask, tokenizer, top_k=50, top_p=1.0, max_length=20):
    """Samples from BOS until every row has drawn EOS or max_length is reached, each token from softmax(top-k / top-p filtered
    logits) at temperature 1 with no min_length ban and no score processors.  Returns (decoder_input_ids [B, L],
    sum_logprobs [B, 1]): per row the sum of log_softmax(filtered logits)[token] over its tokens up to and including EOS
    (finished rows are fed pad tokens and add nothing), not length-normalised.
    One generate(do_sample=True, num_beams=1, return_logprobs=True) call: the KV-cached decode loop with the device sampler
    instead of the reference's uncached forward per step.  The one difference from the reference: the values are returned
    without an autograd graph (generate runs under no_grad), so they can weigh or rank samples but not be differentiated."""
    ids, logprobs = model.generate(
        input_ids=input_ids, image_features=image_features, attention_mask=attention_mask, do_sample=True, num_beams=1,
        return_logprobs=True, top_k=top_k, top_p=top_p, max_length=max_length, temperature=1.0, min_length=0,
        num_return_sequences=1, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None,
        decoder_start_token_id=tokenizer.bos_token_id, pad_token_id=tokenizer.pad_token_id, eos_token_id=tokenizer.eos_token_id)
    return ids, logprobs.sum_logprobs.unsqueeze(1)
