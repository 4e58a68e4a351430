"""Numpy model of the reference's frame stacking (nclone/gym_environment/frame_stack_wrapper.py), batched over envs.

Per env and stacked key, a window of K entries, oldest first:
  - reset (reset(), _reset_to_checkpoint_from_wrapper(), and here the kernel's auto-reset): K - 1 padding entries -- zeros
    ("zero") or copies of the new observation ("repeat") -- then the new observation (frame_stack_wrapper.py:183-224,
    225-264: the deque is cleared, padded, and observation() appends the real entry);
  - any other observation: the oldest entry drops out and the new one is appended (deque(maxlen=K), :123-129, :334-338);
  - terminal stack (this project's info["terminal_game_state_stack"]): for an env reset in this step, the window it would have
    shown at its terminal step -- the last K - 1 entries of its previous window, then its terminal observation; else the
    live window.
tests/test_frame_stack_host.py pins this model to tests/golden/stack.npz (the wrapper itself, run by make_golden_stack.py).
"""
import numpy as np


class StackModel:
    def __init__(self, k, padding="zero"):
        assert 1 <= k <= 12 and padding in ("zero", "repeat")
        self.k, self.repeat = int(k), padding == "repeat"
        self.s = None

    def push(self, x, reset, terminal=None):
        """x: [N, ...] this step's observations; reset: bool [N]; terminal: optional [N, ...] terminal observations of the
        reset envs.  Returns the new windows [N, K, ...] (and, with `terminal`, the terminal windows)."""
        x = np.asarray(x)
        reset = np.asarray(reset, dtype=bool)
        if self.s is None:
            self.s = np.zeros((x.shape[0], self.k) + x.shape[1:], dtype=x.dtype)
        prev = self.s
        new = np.concatenate([prev[:, 1:], x[:, None]], axis=1)
        if reset.any():
            pad = x[reset] if self.repeat else np.zeros_like(x[reset])
            new[reset, : self.k - 1] = pad[:, None]
        self.s = new
        if terminal is None:
            return new
        last = np.where(reset.reshape((-1,) + (1,) * (x.ndim - 1)), np.asarray(terminal), x)
        term = np.concatenate([prev[:, 1:], last[:, None]], axis=1)
        return new, term
