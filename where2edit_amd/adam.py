"""`Adam(params, lr, betas, eps, weight_decay, fused=None)`: torch.optim.Adam's update rule (no amsgrad, no maximize) and its
per-parameter state -- `step` (a float32 CPU scalar tensor), `exp_avg`, `exp_avg_sq` --, so `state_dict()` loads into
`torch.optim.Adam` and back.  The bias corrections and the step size are host arithmetic; the per-element update of every
parameter at the same `step` is ONE launch of libw2e.so's w2e_adam_step (csrc/adam.hip) when all its tensors are contiguous fp32
tensors on one GPU.  Everything else (CPU tensors, other dtypes, strided gradients) takes multi-tensor (`torch._foreach_*`)
updates, the operations of torch's own single-tensor form in the same order.  The optimizer of the region-attention loop
(attention/run_attention.py:1051); works under `GradScaler.step` unchanged (it has no `_step_supports_amp_scaling`: the scaler
unscales, checks and calls `step()` or skips it)."""
import torch
from torch.optim.optimizer import Optimizer

from ._fused_opt import FusedStep


class Adam(FusedStep, Optimizer):
    _fused_entry = "w2e_adam_step"
    _fused_state = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, fused=None):
        """`fused`: None = the one-launch kernel wherever it applies, False = never, True = raise where it does not apply."""
        if amsgrad:
            raise ValueError("where2edit_amd.Adam: amsgrad=True is not supported (use torch.optim.Adam)")
        if maximize:
            raise ValueError("where2edit_amd.Adam: maximize=True is not supported (use torch.optim.Adam)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)  # torch.optim.Adam's group keys
        super().__init__(params, defaults)
        self.fused = fused

    @staticmethod
    def _scalars(group, step):
        """adam.py (_single_tensor_adam): step_size = lr / (1 - beta1^step), bias_correction2_sqrt = sqrt(1 - beta2^step)."""
        beta1, beta2 = group["betas"]
        return group["lr"] / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5

    def _fused_update(self, group, step, params):
        beta1, beta2 = group["betas"]
        step_size, bc2_sqrt = self._scalars(group, step)
        self._fused_call(params, (torch.Tensor.numel,), (float(beta1), float(beta2), float(group["eps"]), float(step_size),
                                                          float(bc2_sqrt), float(group["weight_decay"])))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1  # (a CPU tensor: reading it back is no device synchronisation)
                by_step.setdefault(float(state["step"]), []).append(p)
            for step, params in by_step.items():
                if self._fused_applies(params):
                    self._fused_update(group, step, params)
                    continue
                grads = [p.grad for p in params]
                if group["weight_decay"] != 0:
                    grads = torch._foreach_add(grads, params, alpha=group["weight_decay"])
                exp_avg = [self.state[p]["exp_avg"] for p in params]
                exp_avg_sq = [self.state[p]["exp_avg_sq"] for p in params]
                step_size, bc2_sqrt = self._scalars(group, step)
                torch._foreach_lerp_(exp_avg, grads, 1 - beta1)
                torch._foreach_mul_(exp_avg_sq, beta2)
                torch._foreach_addcmul_(exp_avg_sq, grads, grads, value=1 - beta2)
                denom = torch._foreach_sqrt(exp_avg_sq)
                torch._foreach_div_(denom, bc2_sqrt)
                torch._foreach_add_(denom, group["eps"])
                torch._foreach_addcdiv_(params, exp_avg, denom, value=-step_size)
        return loss
