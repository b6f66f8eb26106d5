"""Several samples per observation from the flow head, one chosen on the device (fv_head_set_flow_samples / fv_head_flow_sample_multi): the host-side
checks and the coherence score's weight schedule.

A call draws S candidates per observation (candidate s is the single-sample call at offset + (s << 56), so candidate 0 is today's sample) and returns ONE:
    "first"     candidate 0
    "medoid"    the candidate with the smallest sum of squared distances to the others: the one the rest agree with
    "coherent"  the candidate that best continues the previous chunk over the steps the two share, step k weighted decay**k (the backward-coherence
                criterion of Bidirectional Decoding, Liu et al. 2024); a row without a previous chunk takes the medoid
The mean of the candidates is not offered: between two modes of the learned distribution it is a chunk that belongs to neither."""
from typing import List, Optional, Tuple

FLOW_SAMPLES_MAX = 16                         # FV_FLOW_SAMPLES_MAX
FLOW_SELECTS = ("first", "medoid", "coherent")


def check_flow_samples(samples) -> int:
    """-> samples as an int 1 .. 16; ValueError naming flow_samples otherwise (bool and non-integers included)"""
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= FLOW_SAMPLES_MAX:
        raise ValueError(f"flow_samples must be an integer 1 .. {FLOW_SAMPLES_MAX}, got {samples!r}")
    return samples


def check_flow_select(samples, select: Optional[str], *, action_head: str = "flow", chunk_size: Optional[int] = None,
                      rtc_method: Optional[str] = None) -> Tuple[int, Optional[str]]:
    """The settings of a policy that samples several candidates, checked together before any engine exists -> (samples, select); select is None with one
    sample and "medoid" when several are asked for without a name.  ValueError naming both settings for: a regression head; samples outside 1 .. 16; a
    select name with one sample; an unknown name; "coherent" with chunk_size = 1 (nothing to continue); rtc_method = "guidance" with several samples."""
    if action_head != "flow" and (samples not in (None, 1) or select is not None):
        raise ValueError(f"flow_samples={samples!r} / flow_select={select!r} need action_head='flow', got action_head={action_head!r}")
    samples = check_flow_samples(1 if samples is None else samples)
    if select is not None and select not in FLOW_SELECTS:
        raise ValueError(f"flow_select must be one of {list(FLOW_SELECTS)}, got {select!r} (flow_samples={samples})")
    if samples == 1:
        if select is not None:
            raise ValueError(f"flow_select={select!r} chooses among several candidates, but flow_samples=1")
        return 1, None
    select = "medoid" if select is None else select
    if select == "coherent" and chunk_size is not None and chunk_size < 2:
        raise ValueError(f"flow_select='coherent' with flow_samples={samples} scores the steps a chunk shares with the previous one: chunk_size={chunk_size} has none")
    if rtc_method == "guidance":
        raise ValueError(f"flow_samples={samples} with rtc_method='guidance': guided sampling with candidates is not offered (use flow_select='coherent' or rtc_method='prefix')")
    return samples, select


def coherence_weights(K: int, decay: float = 0.5) -> List[float]:
    """w[k] = decay**k for the K steps of a chunk: the steps executed first count most.  0 < decay <= 1."""
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"coherence_weights: K must be a positive integer, got {K!r}")
    decay = float(decay)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"flow_coherence_decay must lie in (0, 1], got {decay!r}")
    return [decay ** k for k in range(K)]
