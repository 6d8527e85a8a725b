"""numpy restatement of what the reference's BAIRPushingDataset returns for a sample (vp_suite/datasets/bair.py:55-63) apart from the
frames' preprocess() (tests/frames_ref.py restates that): the two slices and the float32 cast."""
import numpy as np


def seq_len(n_frames, seq_step):
    """base_dataset.py:165-187."""
    return (n_frames - 1) * seq_step + 1


def sample(obs, actions, n_frames, seq_step):
    """(obs[:seq_len:seq_step], actions[:seq_len:seq_step].float()) of ONE stored sequence: obs [t, h, w, c], actions [t, a]."""
    n = seq_len(n_frames, seq_step)
    return obs[:n:seq_step], actions[:n:seq_step].astype(np.float32)


def gather(actions, seqs, n_frames, seq_step):
    """float32 [B, n_frames, A]: the action halves of sample() for the stored sequences `seqs` out of actions [N, T', A]."""
    return np.stack([sample(actions[s], actions[s], n_frames, seq_step)[1] for s in seqs])
