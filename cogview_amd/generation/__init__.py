"""Incremental decoding on the HIP model: the reference's generation/sampling.py surface."""
from .decoder import GraphDecoder, SamplingDecoder                                        # noqa: F401
from .id_space import IdSpace                                                              # noqa: F401
from .sampling import (DeviceBatchFiller, DeviceFiller, DeviceGenerator, add_interlacing_beam_marks, filling_sequence,    # noqa: F401
                       generate_batch_on_device, generate_on_device, get_batch, inverse_prompt_score,
                       inverse_prompt_score_on_device, magnify, magnify_batch, plan_chunk_steps, plan_device_batch,
                       plan_device_batch_fill, plan_device_fill, plan_device_generation, post_selection_rows, rerank_generated,
                       shrink_beams, top_k_logits)
