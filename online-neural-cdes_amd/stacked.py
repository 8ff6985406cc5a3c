"""``StackedNeuralCDE``: drop-in for the reference's stacked model (src/ncde/stacked.py:7-131 of the reference tree).

A chain of Neural CDEs, dZ_1 = f_1(Z_1) dX, dZ_2 = f_2(Z_2) dZ_1, ...: layer i returns its whole hidden sequence and layer
i + 1 reads it as the linear coefficients of its control.  Same constructor arguments, same ``state_dict`` keys
(``ncdes.{i}.*``, ``fc_output.*``) and same ``forward`` as the reference.  With ``adjoint=False`` the coefficients of every
layer but the first require grad; ``cdeint`` then runs ``ncde_backward_control`` (solver.py), which returns dL/dcoeffs from the
fused backward, so the whole stack trains on the fused kernels.  With ``adjoint=True`` the inner sequences receive no gradient
through the solve (the reference's warning, torchcde/solver.py:207-221).
"""
from torch import nn

from .ncde import NeuralCDE


class StackedNeuralCDE(nn.Module):
    def __init__(self, input_dim, hidden_dims, output_dim, hidden_hidden_dim=15, static_dim=None, adjoint=True,
                 return_sequences=False, static_in_all_layers=False):
        assert isinstance(hidden_dims, list), "hidden_dims must be a list, got type {}".format(type(hidden_dims))
        super().__init__()
        self.input_dim, self.hidden_dims, self.output_dim = input_dim, hidden_dims, output_dim
        self.hidden_hidden_dim = hidden_hidden_dim      # (kept, not used: the reference builds every layer with NeuralCDE's default)
        self.static_dim = static_dim
        self.adjoint = adjoint
        self.return_sequences = return_sequences
        self.static_in_all_layers = static_in_all_layers
        self.num_stacked = len(hidden_dims)

        # inner layers return their sequence without a final linear; the last one applies its final linear (stacked.py:64-85)
        self.ncdes = nn.ModuleList()
        input_, static_ = input_dim, static_dim
        for i, hidden_ in enumerate(hidden_dims):
            last = i == self.num_stacked - 1
            self.ncdes.append(self._create_ncde(input_, hidden_, output_dim, static_, last, self.return_sequences if last else True))
            input_ = hidden_
            if not self.static_in_all_layers:
                static_ = None
        self.fc_output = nn.Linear(hidden_dims[-1], output_dim)      # exists, unused: as in the reference (stacked.py:88)

    def _create_ncde(self, input_dim, hidden_dim, output_dim, static_dim, apply_final_linear, return_sequences):
        return NeuralCDE(input_dim, hidden_dim, output_dim, static_dim, use_initial=True, interpolation="linear",
                         adjoint=self.adjoint, num_layers=3, apply_final_linear=apply_final_linear,
                         return_sequences=return_sequences)

    def _handle_hidden_static_features(self, x, hidden_state):
        if self.static_dim is None or not self.static_in_all_layers:
            return hidden_state
        return [x[0], hidden_state]

    def online(self, batch_size, *, initial_value_if_nan=0.0, one_launch=False):
        """A handle that carries every layer's state of ``batch_size`` streams from one observation to the next (online.py):
        ``step(x_new)`` answers what ``return_sequences=True`` on the whole prefix gives at the newest knot.  Over this module's own
        parameters (no copies).  one_launch=True: all layers in one launch of ncde_stream_stack_step instead of one launch per layer
        (the same bits; measured slower per call, hence not the default)."""
        from .online import OnlineStackedNeuralCDE
        return OnlineStackedNeuralCDE(self, batch_size, initial_value_if_nan=initial_value_if_nan, one_launch=one_launch)

    def forward(self, x):
        hidden_state = self.ncdes[0](x)
        for ncde in self.ncdes[1:]:
            hidden_state = ncde(self._handle_hidden_static_features(x, hidden_state))
        return hidden_state
