"""numpy fp64 oracle of iPNDM (diffusers' PNDMScheduler with ``skip_prk_steps``), written as the plain list-based ``step_plms`` in diffusers'
operation order.

Test infrastructure: shares no code with consolver_amd/scheduling_pndm.py or the kernel, and does not use the collapsed linear
coefficients -- every step keeps the list ``ets``, forms the Adams-Bashforth combination as diffusers 0.26.3 writes it (from
memory) and applies the transfer formula of ``_get_prev_sample``.  The beta table comes from oracle/solver_oracle.py, which
tests/golden pins to the reference.
"""
import numpy as np

from oracle import solver_oracle as so


def ddim_transfer(x, eps, a_t, a_p):
    """the eta = 0 DDIM transfer from cumulative alpha a_t to a_p, the way the DDIM scheduler writes it"""
    x0 = (x - np.sqrt(1.0 - a_t) * eps) / np.sqrt(a_t)
    return np.sqrt(a_p) * x0 + np.sqrt(1.0 - a_p) * eps


class PNDMOracle:
    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear", skip_prk_steps=False,
                 set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading", steps_offset=0):
        assert skip_prk_steps and prediction_type in ("epsilon", "v_prediction") and timestep_spacing == "leading"
        self.T = num_train_timesteps
        self.ac = so.alphas_cumprod(so.make_betas(beta_schedule, beta_start, beta_end, num_train_timesteps)).astype(np.float64)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else self.ac[0]
        self.prediction_type, self.steps_offset = prediction_type, steps_offset

    def set_timesteps(self, n):
        self.n = n
        step_ratio = self.T // n
        _timesteps = (np.arange(0, n) * step_ratio).round() + self.steps_offset
        self.timesteps = np.concatenate([_timesteps[:-1], _timesteps[-2:-1], _timesteps[-1:]])[::-1].astype(np.int64)
        self.ets = []
        self.counter = 0
        self.cur_sample = None

    def get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        alpha_prod_t = self.ac[timestep]
        alpha_prod_t_prev = self.ac[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        if self.prediction_type == "v_prediction":
            model_output = (alpha_prod_t ** 0.5) * model_output + (beta_prod_t ** 0.5) * sample
        sample_coeff = (alpha_prod_t_prev / alpha_prod_t) ** 0.5
        model_output_denom_coeff = alpha_prod_t * beta_prod_t_prev ** 0.5 + (alpha_prod_t * beta_prod_t * alpha_prod_t_prev) ** 0.5
        return sample_coeff * sample - (alpha_prod_t_prev - alpha_prod_t) * model_output / model_output_denom_coeff

    def step(self, model_output, sample):
        model_output, sample = np.asarray(model_output, np.float64), np.asarray(sample, np.float64)
        timestep = int(self.timesteps[self.counter])
        prev_timestep = timestep - self.T // self.n
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep = timestep
            timestep = timestep + self.T // self.n
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(self.ets) == 1 and self.counter == 1:
            model_output = (model_output + self.ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            model_output = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            model_output = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4])
        prev_sample = self.get_prev_sample(sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return prev_sample
