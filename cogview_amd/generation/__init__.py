"""Incremental decoding on the HIP model: the reference's generation/sampling.py surface."""
from .decoder import GraphDecoder, SamplingDecoder                                        # noqa: F401
from .id_space import IdSpace                                                              # noqa: F401
from .sampling import (DeviceFiller, add_interlacing_beam_marks, filling_sequence, generate_on_device,  # noqa: F401
                       get_batch, inverse_prompt_score, magnify, plan_device_fill, plan_device_generation, shrink_beams,
                       top_k_logits)
