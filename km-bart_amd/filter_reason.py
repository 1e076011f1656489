"""Perplexity filter driver: counterpart of the reference's scripts/filter_reason.py (flags of filter_reason.py:102-136).
Loads a checkpoint, scores every record of "reason_<split>.json" with `src.scoring.perplexity_filter` and writes the records whose
log-perplexity is below --pp_threshold to "<output_dir>/reason_<split>.json", the reference's output.  `--data_dir DIR` reads the
reference's file format (tokenizer: the BART-large files on disk or `--tokenizer_json`); `--synthetic N` needs no files: N synthetic
batches, and the records written are `{"index": i}` for the kept samples."""
import argparse
import json
import os
import sys
from datetime import datetime

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartForConditionalGeneration  # noqa: E402
from src.scoring import perplexity_filter  # noqa: E402
from src.utils import Logger  # noqa: E402


def main(args):
    device = torch.device("cuda", 0)
    logger = Logger(args.log_dir)
    logger.info("Loading model...")
    model = MultiModalBartForConditionalGeneration.from_pretrained(args.checkpoint)
    model.to(device)
    logger.info('Loaded model from "{}"'.format(args.checkpoint))
    logger.info("Loading data...")
    if args.synthetic > 0:
        loader = []
        for i in range(args.synthetic):
            b = make_batch(args.batch_size, seed=4321 + i)
            b["dataset_index"] = [i * args.batch_size + j for j in range(args.batch_size)]
            loader.append(b)
        total = args.synthetic * args.batch_size

        def raw(i):
            return {"index": i}
    else:
        from torch.utils.data import DataLoader
        from src.data.collation import Collator
        from src.data.dataset import ReasonDataset
        from src.data.offline_tokenizer import load_base_tokenizer
        from src.data.tokenization import ConditionTokenizer
        tokenizer = ConditionTokenizer(base_tokenizer=load_base_tokenizer(args.tokenizer_json or "facebook/bart-large"))
        dataset = ReasonDataset(args.data_dir, split=args.split)
        loader = DataLoader(dataset, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers,
                            collate_fn=Collator(tokenizer, has_label=True, pin_memory=args.num_workers == 0))
        total = len(dataset)
        raw = dataset.get_raw_data
    start = datetime.now()
    logger.info("Start computing score", pad=True)
    kept = perplexity_filter(model, loader, device, args, logger)
    logger.info("Filtering complete in: " + str(datetime.now() - start), pad=True)
    logger.info("Saving results...")
    records = [raw(i) for i in kept]
    os.makedirs(args.output_dir, exist_ok=True)
    with open(os.path.join(args.output_dir, "reason_{}.json".format(args.split)), "w") as f:
        json.dump(records, f)
    logger.info("Remaining {}/{}".format(len(records), total))
    logger.info('Saved results in "{}"'.format(args.output_dir))


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", default=None, type=str, help="directory of reason_<split>.json and the feature files")
    p.add_argument("--output_dir", required=True, type=str, help="directory the filtered reason_<split>.json is written to")
    p.add_argument("--checkpoint", required=True, type=str, help="checkpoint directory to load the model from")
    p.add_argument("--log_dir", default=None, type=str, help="also log to files there")
    p.add_argument("--split", default="train", type=str)
    p.add_argument("--pp_threshold", default=3.5, type=float, help="keep a sample when log(perplexity) is below this")
    p.add_argument("--cpu", action="store_true")
    p.add_argument("--amp", action="store_true")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--num_workers", type=int, default=0)
    p.add_argument("--synthetic", type=int, default=0, help="score N synthetic batches instead of files")
    p.add_argument("--tokenizer_json", default=None, type=str)
    p.set_defaults(use_event=True, use_image=True)
    args = p.parse_args(argv)
    if args.cpu:
        raise ValueError("--cpu: this build has no CPU path")
    if args.synthetic <= 0 and args.data_dir is None:
        raise ValueError("give --data_dir or --synthetic N")
    return args


if __name__ == "__main__":
    main(parse_args())
