"""Sequence-level rewards computed on the device, for `src.training.self_critical_step`.

`CiderReward` scores sampled token ids with CIDEr-D (Vedantam et al. 2015, the consensus reward of self-critical sequence
training, Rennie et al. 2017) or plain CIDEr against reference tables resident in device memory: one launch per [B, L] id
matrix (kmb_cider_reward, csrc/cider_reward.hip), nothing read back.

This is a TOKEN-ID-level reward.  The reference's evaluation (validate_generation_score: PTB tokenisation, word n-grams,
Java scorers) works on words; the numbers are not comparable, and nothing here is an evaluation metric.

The definition.  Tokens of a row (`reward_tokens`): column 0 (the decoder start token) is skipped, the row stops in front of
the first eos behind it, every pad and bos is dropped; a reference's label ids get a start token in front and go through the
same rule.  Corpus: N items, item i with m_i >= 0 references; df_n(w) = number of items with a reference holding n-gram w,
idf_n(w) = log N - log max(1, df_n(w)) (log N for an n-gram in no reference).  g_x,n(w) = count_x(w) idf_n(w);
s_n(h, r) = sum_{w in h} num / (||g_h,n|| ||g_r,n||), 0 when a norm is 0, with num = min(g_h, g_r) g_r (CIDEr-D) or g_h g_r
(CIDEr); pen = exp(-(L_h - L_r)^2 / (2 sigma^2)) (CIDEr-D, sigma 6) or 1; score = (10 / m_i) sum_r pen 1/4 sum_{n=1..4} s_n.

Limits: vocab_size <= 65536 (a token is a 16-bit slot of a 64-bit n-gram key) and id matrices of at most MAX_T = 256
columns (KMB_CIDER_MAX_T, csrc/cider_reward.h)."""
import ctypes as C

import numpy as np
import torch

ORDERS = 4
MAX_T = 256                 # KMB_CIDER_MAX_T (csrc/cider_reward.h)
MAX_VOCAB = 65536
VARIANTS = {"D": 0, "plain": 1}


def reward_tokens(row, pad, bos, eos):
    """The scored tokens of an id row: without column 0, up to the first `eos` behind it, without `pad` and `bos` (and without
    ids outside [0, 65536), which have no key)."""
    out = []
    for v in list(row)[1:]:
        v = int(v)
        if v == eos:
            break
        if v != pad and v != bos and 0 <= v < MAX_VOCAB:
            out.append(v)
    return out


def _distinct(a, b):
    """starts of the runs of equal (a, b) pairs in two aligned sorted arrays"""
    new = np.ones(len(a), dtype=bool)
    new[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    return np.flatnonzero(new)


def build_cider_tables(groups, vocab_size):
    """The reference tables of kmb_cider_reward from `groups`, a list over items of lists of references, each a list of token ids
    (already stripped: reward_tokens).  Pure numpy on the host; returns a dict of numpy arrays and two scalars:

      n_items N, idf_miss = float32(log N)
      df_keys uint64 [E_df], df_idf float32 [E_df], df_offsets int64 [5]: order n's distinct n-grams in
          [df_offsets[n - 1], df_offsets[n]), ascending unsigned; idf = log N - log max(1, df) in float64, then rounded
      item_ref_offsets int32 [N + 1], ref_len int32 [R]
      ref_norm float32 [R, 4] (sum and sqrt in float64, then rounded)
      ref_ng_offsets int32 [4 R + 1]: slice 4 r + (n - 1) of ref_keys uint64 / ref_w float32 [E_ref] (count * idf), ascending
          unsigned within a slice

    An n-gram is the key sum_k tok[k] << 16 (n - 1 - k): the first token in the highest of the n used 16-bit slots, one key
    space per order, compared UNSIGNED (a 4-gram whose first token is >= 32768 has the top bit set).
    Size: 12 (E_df + E_ref) + 36 R + 4 N + 8 bytes, E_ref = sum over references of their distinct n-grams <= sum_r (4 L_r - 6),
    E_df = the corpus' distinct n-grams <= E_ref -- a few hundred MB for 1.2 M references of ~10 tokens.
    Raises ValueError for vocab_size > 65536, an empty corpus or a token outside [0, vocab_size)."""
    vocab_size = int(vocab_size)
    if vocab_size < 1 or vocab_size > MAX_VOCAB:
        raise ValueError("build_cider_tables: vocab_size must be in [1, 65536] (a token is a 16-bit slot of the key), got %d" % vocab_size)
    N = len(groups)
    if N < 1:
        raise ValueError("build_cider_tables: no items")
    per_item = np.array([len(g) for g in groups], dtype=np.int64)
    R = int(per_item.sum())
    if R >= 2 ** 29:
        raise ValueError("build_cider_tables: too many references for 32-bit offsets")
    item_ref_offsets = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(per_item, out=item_ref_offsets[1:])
    ref_item = np.repeat(np.arange(N, dtype=np.int64), per_item)
    refs = [r for g in groups for r in g]
    ref_len = np.array([len(r) for r in refs], dtype=np.int64)
    tok = np.fromiter((t for r in refs for t in r), dtype=np.int64, count=int(ref_len.sum()))
    if tok.size and (int(tok.min()) < 0 or int(tok.max()) >= vocab_size):
        raise ValueError("build_cider_tables: a reference token lies outside [0, %d)" % vocab_size)
    ref_start = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(ref_len, out=ref_start[1:])
    ref_of_tok = np.repeat(np.arange(R, dtype=np.int64), ref_len)
    left = ref_len[ref_of_tok] - (np.arange(tok.size, dtype=np.int64) - ref_start[ref_of_tok])   # tokens from here to the reference's end
    utok = tok.astype(np.uint64)
    log_n = np.log(np.float64(N))

    df_keys, df_idf, df_offsets = [], [], np.zeros(ORDERS + 1, dtype=np.int64)
    per_order = []                                   # (reference, key, weight float64) of each order, sorted by (reference, key)
    counts = np.zeros((R, ORDERS), dtype=np.int64)   # distinct n-grams of a reference
    norm_sq = np.zeros((R, ORDERS), dtype=np.float64)
    for n in range(1, ORDERS + 1):
        at = np.flatnonzero(left >= n)
        key = np.zeros(at.size, dtype=np.uint64)
        for k in range(n):
            key = (key << np.uint64(16)) | utok[at + k]
        r = ref_of_tok[at]
        order = np.lexsort((key, r))
        r, key = r[order], key[order]
        starts = _distinct(r, key)
        mult = np.diff(np.append(starts, r.size))
        r, key = r[starts], key[starts]              # the distinct n-grams of every reference
        item = ref_item[r]
        order = np.lexsort((item, key))
        k2, i2 = key[order], item[order]
        dfk, dfc = np.unique(k2[_distinct(k2, i2)], return_counts=True)   # items holding the n-gram; ascending unsigned
        idf = log_n - np.log(np.maximum(1, dfc).astype(np.float64))
        w = mult.astype(np.float64) * idf[np.searchsorted(dfk, key)]
        df_keys.append(dfk)
        df_idf.append(idf.astype(np.float32))
        df_offsets[n] = df_offsets[n - 1] + dfk.size
        counts[:, n - 1] = np.bincount(r, minlength=R)
        norm_sq[:, n - 1] = np.bincount(r, weights=w * w, minlength=R)
        per_order.append((r, key, w))

    total = int(counts.sum())
    if total >= 2 ** 31:
        raise ValueError("build_cider_tables: %d reference n-grams do not fit 32-bit offsets" % total)
    ref_ng_offsets = np.zeros(ORDERS * R + 1, dtype=np.int64)
    np.cumsum(counts.reshape(-1), out=ref_ng_offsets[1:])
    ref_keys = np.zeros(total, dtype=np.uint64)
    ref_w = np.zeros(total, dtype=np.float32)
    for n, (r, key, w) in enumerate(per_order):
        first = np.zeros(R + 1, dtype=np.int64)      # where a reference's run starts inside this order's arrays
        np.cumsum(counts[:, n], out=first[1:])
        dst = ref_ng_offsets[ORDERS * r + n] + (np.arange(r.size, dtype=np.int64) - first[r])
        ref_keys[dst] = key
        ref_w[dst] = w.astype(np.float32)
    return {
        "n_items": N,
        "idf_miss": np.float32(log_n),
        "df_keys": np.concatenate(df_keys) if df_keys else np.zeros(0, dtype=np.uint64),
        "df_idf": np.concatenate(df_idf) if df_idf else np.zeros(0, dtype=np.float32),
        "df_offsets": df_offsets,
        "item_ref_offsets": item_ref_offsets.astype(np.int32),
        "ref_len": ref_len.astype(np.int32),
        "ref_norm": np.sqrt(norm_sq).astype(np.float32),
        "ref_ng_offsets": ref_ng_offsets.astype(np.int32),
        "ref_keys": ref_keys,
        "ref_w": ref_w,
    }


def _upload(a, device):
    """a table on the device; uint64 keys as their int64 bit patterns, an empty table as one zero element (a real allocation)"""
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class CiderReward:
    """CIDEr-D (variant="D") or plain CIDEr (variant="plain") over token ids, on the device.

    groups: list over items of lists of references, each a list of token ids already stripped by `reward_tokens`.
    reward(ids, item_of_row) -> float32 [B] on the device, one launch, no synchronisation."""

    def __init__(self, groups, vocab_size, pad_token_id, bos_token_id, eos_token_id, variant="D", sigma=6.0, device="cuda",
                 group_keys=None):
        if variant not in VARIANTS:
            raise ValueError("CiderReward: variant must be 'D' or 'plain', got %r" % (variant,))
        if not float(sigma) > 0.0:
            raise ValueError("CiderReward: sigma must be > 0, got %r" % (sigma,))
        self.variant, self.sigma = variant, float(sigma)
        self.pad_token_id, self.bos_token_id, self.eos_token_id = int(pad_token_id), int(bos_token_id), int(eos_token_id)
        self.device = torch.device(device)
        self.tables = build_cider_tables(groups, vocab_size)
        t = self.tables
        self.n_items, self.n_refs, self.n_ref_entries = int(t["n_items"]), int(t["ref_len"].size), int(t["ref_keys"].size)
        self._df_offsets = (C.c_int64 * (ORDERS + 1))(*[int(x) for x in t["df_offsets"]])
        self._dev = {k: _upload(t[k], self.device) for k in ("df_keys", "df_idf", "item_ref_offsets", "ref_len", "ref_norm",
                                                             "ref_ng_offsets", "ref_keys", "ref_w")}
        self.device = self._dev["ref_len"].device    # with its index: "cuda" became the current device, which is what tensors report
        keys = list(range(self.n_items)) if group_keys is None else list(group_keys)
        if len(keys) != self.n_items:
            raise ValueError("CiderReward: %d group keys for %d items" % (len(keys), self.n_items))
        self.item_of_group = {k: i for i, k in enumerate(keys)}
        if len(self.item_of_group) != self.n_items:
            raise ValueError("CiderReward: group keys repeat")

    def table_bytes(self):
        return sum(v.numel() * v.element_size() for v in self._dev.values())

    @classmethod
    def from_records(cls, records, tokenizer, config, variant="D", sigma=6.0, device="cuda", lm_max_len=30, chunk=4096):
        """References from dataset records ({"index", "task_type", "labels", ...}, src/data/dataset.py): grouped by
        (record["index"], record["task_type"]) -- the refs_list[index][relation] of the reference's evaluation -- with `labels`
        tokenised as the Collator tokenises a training target (clipped to lm_max_len BPE tokens, encode_label), a start token in
        front and reward_tokens applied.  The (index, task_type) -> item map is `item_of_group`; `for_batch` resolves through it.
        A record without an `index` raises ValueError."""
        from src.data.collation import Collator
        col = Collator(tokenizer, has_label=True, lm_max_len=lm_max_len)
        pad, bos, eos = int(config.pad_token_id), int(config.bos_token_id), int(config.eos_token_id)
        start = getattr(config, "decoder_start_token_id", None)
        start = eos if start is None else int(start)
        records = [r for r in records if r is not None]
        item_of, groups = {}, []
        for lo in range(0, len(records), chunk):
            part = records[lo:lo + chunk]
            target = col._clip_texts([r["labels"] for r in part], lm_max_len)
            rows = tokenizer.encode_label(label=target)["labels"].tolist()
            for r, row in zip(part, rows):
                if r.get("index") is None:
                    raise ValueError("CiderReward.from_records: a record without an `index` (its references have no group)")
                key = (r["index"], r["task_type"])
                if key not in item_of:
                    item_of[key] = len(groups)
                    groups.append([])
                groups[item_of[key]].append(reward_tokens([start] + row, pad, bos, eos))
        return cls(groups, config.vocab_size, pad, bos, eos, variant=variant, sigma=sigma, device=device, group_keys=list(item_of))

    def reward(self, ids, item_of_row, out=None):
        """ids int64 [B, L] (L <= 256, unit column stride) and item_of_row int32 [B], both on the reward's device -> float32 [B]
        there (written into `out`'s first B words when given).  An item outside [0, n_items) scores 0.  Enqueued on the current
        stream; nothing is read back."""
        from kmbart._lib import check, load, ptr
        if ids.device != self.device or item_of_row.device != self.device:
            raise ValueError("CiderReward.reward: ids and item_of_row must be on %s" % self.device)
        if ids.dtype != torch.int64 or ids.dim() != 2 or (ids.shape[1] > 1 and ids.stride(1) != 1):
            raise ValueError("CiderReward.reward: ids must be int64 [B, L] with unit column stride")
        B, L = ids.shape
        if item_of_row.dtype != torch.int32 or item_of_row.shape != (B,) or not item_of_row.is_contiguous():
            raise ValueError("CiderReward.reward: item_of_row must be contiguous int32 [B]")
        if self.device.type != "cuda":
            raise RuntimeError("CiderReward.reward runs on the MI355X only (the tables are on %s): there is no host path" % self.device)
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        elif out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < B:
            raise ValueError("CiderReward.reward: out must be contiguous float32 with at least B elements on %s" % self.device)
        if B == 0:
            return out
        ld = int(ids.stride(0)) if B > 1 else max(int(ids.stride(0)), L)
        if L < 1 or ld < L:
            raise ValueError("CiderReward.reward: ids needs at least one column and a row stride >= L")
        d = self._dev
        with torch.cuda.device(self.device):
            check(load().kmb_cider_reward(
                ptr(ids), ld, B, L, self.pad_token_id, self.bos_token_id, self.eos_token_id,
                ptr(item_of_row), self.n_items, ptr(d["df_keys"]), ptr(d["df_idf"]), C.cast(self._df_offsets, C.c_void_p),
                float(self.tables["idf_miss"]), ptr(d["item_ref_offsets"]), self.n_refs, ptr(d["ref_len"]), ptr(d["ref_norm"]),
                ptr(d["ref_ng_offsets"]), ptr(d["ref_keys"]), ptr(d["ref_w"]), self.n_ref_entries, VARIANTS[self.variant],
                self.sigma, ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def items_for_batch(self, batch, repeats=1):
        """The batch's (index, task_type) pairs as item ids, each `repeats` times in a row (the row order of
        generate(num_return_sequences=repeats)); KeyError for a group the tables do not hold."""
        index, task = batch["index"], batch["task_type"]
        if len(index) != len(task):
            raise ValueError("for_batch: %d indices for %d task types" % (len(index), len(task)))
        items = []
        for key in zip(index, task):
            if key not in self.item_of_group:
                raise KeyError("CiderReward: no references for group %r" % (key,))
            items += [self.item_of_group[key]] * int(repeats)
        return items

    def for_batch(self, batch, repeats=1):
        """`ids -> float32 [B * repeats]` for self_critical_step: the batch's `index` / `task_type` lists are resolved to item ids
        here, on the host, once; the closure only launches."""
        items = torch.tensor(self.items_for_batch(batch, repeats), dtype=torch.int32).to(self.device, non_blocking=True)
        return lambda ids: self.reward(ids, items)
