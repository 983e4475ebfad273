"""Rule-based controllers with the reference's constructors (rl/agents/rule_based.py).

``take_action`` is the host model: numpy, one observation at a time, for ``PedNetParallelEnv`` callers.  The same rules run on the
device for every env through ``VecPedNetEnv.set_controllers`` (pednstream_amd/csrc/pedn_ctrl.hpp), bit for bit: every detail of the
reference's arithmetic is kept on purpose --

  gater      ``np.mean`` of the float32 densities (NumPy's summation order), "open" compared with the literal 2 and answered with the
             links' physical widths, ``current_width +/- 1`` in float32 (a Python int does not widen np.float32), the threshold compared
             in float32;
  separator  the forward link's outflow ``obs[1]``; ``obs[4]`` does not exist in a 4-feature observation, so the reverse term is 0.0;
             float32 arithmetic without smoothing, binary64 over ``float(np.mean(buffer))`` with it; the buffer belongs to the agent
             object (it survives env resets).

Every action is returned as a float32 array.
"""
import numpy as np


class BaseAgent:
    """What every controller offers: ``take_action(obs) -> np.ndarray``."""

    def take_action(self, obs, deterministic=False):
        raise NotImplementedError


class RuleBasedGaterAgent(BaseAgent):
    """Gate widths from the downstream densities: all gates open while the links' mean density is at most 2, otherwise each gate
    one metre wider / narrower than now when its link's density is above / below ``threshold_density`` (its full width when equal)."""

    def __init__(self, outgoing_links, obs_mode, threshold_density=0.8):
        if obs_mode != "option2":
            raise ValueError("RuleBasedGaterAgent requires density information ('obs_mode' must be 'option2') with density observation.")
        self.outgoing_links = outgoing_links
        self.threshold_density = threshold_density
        self.features_per_link = 4          # inflow, reverse outflow, density, current gate width

    def take_action(self, obs, deterministic=False):
        f = self.features_per_link
        densities = [obs[i * f + 2] for i in range(len(self.outgoing_links))]
        avg = np.mean(densities) if densities else 0.0
        if avg <= 2:
            return np.array([link.width for link in self.outgoing_links], dtype=np.float32)
        actions = []
        for i, link in enumerate(self.outgoing_links):
            density, current_width = obs[i * f + 2], obs[i * f + f - 1]
            if density > self.threshold_density:
                actions.append(current_width + 1)
            elif density < self.threshold_density:
                actions.append(current_width - 1)
            else:
                actions.append(link.width)
        return np.array(actions, dtype=np.float32)


class RuleBasedSeparatorAgent(BaseAgent):
    """Lane split of a separator in proportion to the two directions' flows, optionally over a moving average of the last
    ``buffer_size`` observed values."""

    def __init__(self, width, use_smoothing=False, buffer_size=5):
        self.road_width = width
        self.use_smoothing = use_smoothing
        self.buffer_size = buffer_size
        self._link_inflow_buffer = [] if use_smoothing else None
        self._reversed_link_inflow_buffer = [] if use_smoothing else None

    def _update_and_smooth_inflow(self, buffer, current):
        if not self.use_smoothing:
            return current
        buffer.append(current)
        if len(buffer) > self.buffer_size:
            buffer.pop(0)
        return float(np.mean(buffer))

    def take_action(self, obs, deterministic=False):
        forward = obs[1] if len(obs) > 1 else 0.0
        reverse = obs[4] if len(obs) > 4 else 0.0
        if self.use_smoothing:
            forward = self._update_and_smooth_inflow(self._link_inflow_buffer, forward)
            reverse = self._update_and_smooth_inflow(self._reversed_link_inflow_buffer, reverse)
        if forward + reverse == 0:
            action = self.road_width / 2
        else:
            action = self.road_width * forward / (forward + reverse)
        return np.array([action], dtype=np.float32)
