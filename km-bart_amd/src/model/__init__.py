from src.model.config import MultiModalBartConfig
from src.model.model import (GenerationLogprobs, LazyLogits, MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining,
                             MultiModalBartModel, SequenceScore)

__all__ = ["MultiModalBartConfig", "MultiModalBartForConditionalGeneration", "MultiModalBartForPreTraining",
           "MultiModalBartModel", "LazyLogits", "SequenceScore", "GenerationLogprobs"]
