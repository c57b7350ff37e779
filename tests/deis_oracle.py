"""numpy fp64 oracle of DEIS (log-rho multistep, orders 1 to 3), written as the plain step-by-step algorithm in diffusers' operation order.

Test infrastructure: shares no code with consolver_amd/scheduling_deis.py or the kernel, and does not use the collapsed linear
coefficients -- every step converts the model output, keeps a list of converted outputs and evaluates the update as diffusers
0.26.3 writes it (from memory): the first-order update in the lambda form of the DPM-Solver, the second- and third-order updates
as differences of ``ind_fn``, the antiderivative of one Lagrange basis polynomial in log rho.  The scheduler integrates the same
polynomials from three shared antiderivatives instead, so the two derivations check each other (tests/test_deis_oracle.py).
The beta table comes from oracle/solver_oracle.py, which tests/golden pins to the reference.
"""
import numpy as np

from oracle import solver_oracle as so


def expected_orders(solver_order, n, lower_order_final=True):
    """the order of every step, diffusers' rule: lower orders while the history fills, and on the last two steps of a run of fewer than 15"""
    out, lower = [], 0
    for i in range(n):
        final = i == n - 1 and lower_order_final and n < 15
        second = i == n - 2 and lower_order_final and n < 15
        if solver_order == 1 or lower < 1 or final:
            out.append(1)
        elif solver_order == 2 or lower < 2 or second:
            out.append(2)
        else:
            out.append(3)
        if lower < solver_order:
            lower += 1
    return out


class DEISOracle:
    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear", solver_order=2,
                 prediction_type="epsilon", lower_order_final=True, timestep_spacing="linspace", steps_offset=0):
        assert solver_order in (1, 2, 3) and prediction_type in ("epsilon", "v_prediction")
        self.T = num_train_timesteps
        self.ac = so.alphas_cumprod(so.make_betas(beta_schedule, beta_start, beta_end, num_train_timesteps)).astype(np.float64)
        self.solver_order, self.prediction_type, self.lower_order_final = solver_order, prediction_type, lower_order_final
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset

    def set_timesteps(self, n):
        T = self.T
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1]
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1] + self.steps_offset
        else:
            ts = np.round(np.arange(T, 0, -T / n)) - 1
        self.timesteps = ts.astype(np.int64)
        all_sigmas = ((1 - self.ac) / self.ac) ** 0.5
        sig = np.interp(self.timesteps, np.arange(T), all_sigmas)
        self.sigmas = np.concatenate([sig, [all_sigmas[0]]]).astype(np.float32).astype(np.float64)      # the last sigma is that of timestep 0
        self.n = n
        self.step_index = 0
        self.model_outputs = [None] * self.solver_order          # oldest first
        self.lower_order_nums = 0
        self.orders = []

    @staticmethod
    def alpha_sigma(sigma):
        alpha_t = 1.0 / (sigma ** 2 + 1.0) ** 0.5
        return alpha_t, sigma * alpha_t

    def convert_model_output(self, model_output, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index])
        if self.prediction_type == "epsilon":                     # (diffusers goes through x0 and back: the identity)
            return model_output
        return alpha_t * model_output + sigma_t * sample

    def first_order_update(self, m, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index + 1])
        alpha_s, sigma_s = self.alpha_sigma(self.sigmas[self.step_index])
        lambda_t = np.log(alpha_t) - np.log(sigma_t)
        lambda_s = np.log(alpha_s) - np.log(sigma_s)
        h = lambda_t - lambda_s
        return (alpha_t / alpha_s) * sample - (sigma_t * (np.exp(h) - 1.0)) * m

    def second_order_update(self, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index + 1])
        alpha_s0, sigma_s0 = self.alpha_sigma(self.sigmas[self.step_index])
        alpha_s1, sigma_s1 = self.alpha_sigma(self.sigmas[self.step_index - 1])
        m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
        rho_t, rho_s0, rho_s1 = sigma_t / alpha_t, sigma_s0 / alpha_s0, sigma_s1 / alpha_s1

        def ind_fn(t, b, c):
            return t * (-np.log(c) + np.log(t) - 1) / (np.log(b) - np.log(c))
        coef1 = ind_fn(rho_t, rho_s0, rho_s1) - ind_fn(rho_s0, rho_s0, rho_s1)
        coef2 = ind_fn(rho_t, rho_s1, rho_s0) - ind_fn(rho_s0, rho_s1, rho_s0)
        return alpha_t * (sample / alpha_s0 + coef1 * m0 + coef2 * m1)

    def third_order_update(self, sample):
        alpha_t, sigma_t = self.alpha_sigma(self.sigmas[self.step_index + 1])
        alpha_s0, sigma_s0 = self.alpha_sigma(self.sigmas[self.step_index])
        alpha_s1, sigma_s1 = self.alpha_sigma(self.sigmas[self.step_index - 1])
        alpha_s2, sigma_s2 = self.alpha_sigma(self.sigmas[self.step_index - 2])
        m0, m1, m2 = self.model_outputs[-1], self.model_outputs[-2], self.model_outputs[-3]
        rho_t, rho_s0, rho_s1, rho_s2 = sigma_t / alpha_t, sigma_s0 / alpha_s0, sigma_s1 / alpha_s1, sigma_s2 / alpha_s2

        def ind_fn(t, b, c, d):
            numerator = t * (np.log(c) * (np.log(d) - np.log(t) + 1) - np.log(d) * np.log(t) + np.log(d) + np.log(t) ** 2 - 2 * np.log(t) + 2)
            denominator = (np.log(b) - np.log(c)) * (np.log(b) - np.log(d))
            return numerator / denominator
        coef1 = ind_fn(rho_t, rho_s0, rho_s1, rho_s2) - ind_fn(rho_s0, rho_s0, rho_s1, rho_s2)
        coef2 = ind_fn(rho_t, rho_s1, rho_s2, rho_s0) - ind_fn(rho_s0, rho_s1, rho_s2, rho_s0)
        coef3 = ind_fn(rho_t, rho_s2, rho_s0, rho_s1) - ind_fn(rho_s0, rho_s2, rho_s0, rho_s1)
        return alpha_t * (sample / alpha_s0 + coef1 * m0 + coef2 * m1 + coef3 * m2)

    def step(self, model_output, sample, round_m=None):
        """one step; ``round_m``: optional rounding applied to the converted output (the 16-bit history entry of the kernel)."""
        sample = np.asarray(sample, np.float64)
        m = self.convert_model_output(np.asarray(model_output, np.float64), sample)
        if round_m is not None:
            m = np.asarray(round_m(m), np.float64)
        self.model_outputs = self.model_outputs[1:] + [m]
        short = self.lower_order_final and self.n < 15
        lower_final = self.step_index == self.n - 1 and short
        lower_second = self.step_index == self.n - 2 and short
        if self.solver_order == 1 or self.lower_order_nums < 1 or lower_final:
            prev, order = self.first_order_update(m, sample), 1
        elif self.solver_order == 2 or self.lower_order_nums < 2 or lower_second:
            prev, order = self.second_order_update(sample), 2
        else:
            prev, order = self.third_order_update(sample), 3
        self.orders.append(order)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return prev
