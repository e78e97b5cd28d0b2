"""The build's own caller harness: tiny-Llama model + budgets + generate loop (hipGraph decode)."""
from .generation import (GraphedBlockDecoder, GraphedDecoder, TokenScores, TokenTopScores, apply_pattern, apply_pyramid_pattern, decode_n_tokens, decode_one_token,  # noqa: F401
                         generate, greedy, load_model, negotiate_graphed_decoder, normalize_cache_length, perplexity, prefill, sample, setup_caches,
                         token_logprobs, token_top_logprobs)
from .penalties import LogitPenalties  # noqa: F401
from .constraints import LogitConstraints  # noqa: F401
from .model import CONFIGS, ModelArgs, Transformer, find_multiple  # noqa: F401
from .streams import DecodeStreams, GraphedStreamsDecoder, generate_streams  # noqa: F401
from .quantize import (WeightOnlyInt4Linear, WeightOnlyInt4QuantHandler, WeightOnlyInt8Linear,  # noqa: F401
                       WeightOnlyInt8QuantHandler)
