"""What the tests of the fit loop share (tests/test_host_fit.py, test_gpu_fit_track.py, test_gpu_fit.py): the
scripted (loss, acc) sequences of the early-stop rule and the host model run over them.

tests/test_host_fit.py holds `early_stop_rule` to a transcription of model.py:344-359 on these sequences; the GPU tests
then hold the kernel to `early_stop_rule`.
"""
import numpy as np

nan = float("nan")
SCRIPTS = {
    "improves then stalls": [(1.0, 0.3), (0.9, 0.4), (0.95, 0.35), (0.8, 0.5), (0.85, 0.45), (0.9, 0.4), (0.95, 0.3), (0.7, 0.6)],
    "ties in accuracy": [(1.0, 0.5), (0.9, 0.5), (0.9, 0.5), (0.95, 0.5), (0.8, 0.5), (1.2, 0.4), (1.3, 0.4), (1.4, 0.4)],
    "better accuracy, worse loss": [(1.0, 0.3), (1.1, 0.4), (1.2, 0.5), (1.3, 0.2), (0.9, 0.35), (0.5, 0.1), (0.4, 0.1), (0.3, 0.6)],
    "nan loss": [(1.0, 0.3), (nan, 0.4), (nan, 0.2), (0.9, 0.5), (nan, 0.6), (0.5, 0.1), (0.5, 0.1), (0.5, 0.1)],
    "nan accuracy": [(1.0, 0.3), (0.9, nan), (0.8, nan), (0.7, 0.4), (0.6, nan), (0.5, nan), (0.4, nan), (0.3, 0.9)],
    "nan first": [(nan, nan), (nan, 0.0), (1.0, 0.0), (0.5, 0.0), (0.6, 0.0)],
    "never better": [(1.0, 0.0), (2.0, 0.0), (0.5, 0.0), (0.4, 0.0)],
    "zero accuracy start": [(0.5, 0.2), (0.4, 0.1), (0.3, 0.1), (0.2, 0.1), (0.1, 0.1), (0.05, 0.3)],
}
RULE_CASES = [(name, mode, patience) for name in SCRIPTS for mode in ("both", "acc") for patience in (1, 3)]
EXTRA = (0.0, 1.0)                                   # better than anything: a track that is not stopped takes it


def run_rule(seq, mode, patience, extra=3):
    """early_stop_rule over seq at ticks 1, 2, ...; after the sequence `extra` further improving results, which a stopped
    track must ignore.  Returns the track after each update and the ticks at which copy_now was set."""
    from grand_plus_amd import fit as gf
    track, images, copies = gf.new_track(), [], []
    for tick, (loss, acc) in enumerate(list(seq) + [EXTRA] * extra, start=1):
        gf.early_stop_rule(track, loss, acc, tick, mode, patience)
        images.append(dict(track))
        if track["copy_now"]:
            copies.append(tick)
    return images, copies


def bits(track):
    """A track (a dict or a TrackImage) with its floats as bit patterns, so that a NaN equals itself."""
    d = track if isinstance(track, dict) else track._asdict()
    return {k: int(np.float32(v).view(np.int32)) if k in ("best_loss", "best_acc") else int(v) for k, v in d.items()}
