// corbo-hip-stage: name=heading_tie slot=4 kind=state_control_eq rows=1 nx_min=3 nu_min=2
//
// A USER stage EQUALITY that ties a control to a state: a steering law, the second input follows the first one scaled by x[2],
//     e(x, u) = (u[1] - (prm[0] * u[0]) * x[2]) - prm[1] = 0          (operation order as written: prm[0] * u[0], times x[2], subtracted from u[1], minus prm[1])
// -- the NON-INTEGRAL STATE-CONTROL TERM (here of dimension 1) of a user's corbo::StageEqualityConstraint subclass (getNonIntegralStateControlTermDimension /
// computeNonIntegralStateControlTerm: one BinaryVectorVertexEdge on (x_k, u_k) per interval, added with addEqualityEdge in front of the interval's dynamics
// edge, nlp_functions.cpp:109-115, 142-145; finite_differences_grid.cpp:58-61; multiple_shooting_grid.cpp:65-68).  Public id CORBO_HIP_STAGE_FN_USER + slot in
// corbo_hip_problem_desc::stage_eq, parameters stage_eq_params[0..7].  An edge inside the stage block (x_k, u_k): the sweep kernel's extra-edge instantiation
// evaluates it, the block-tridiagonal / band routes factorise.  `value` writes ROWS values; the vertex dimensions are template parameters like the kernels
// instantiate them.  Compiled without floating-point contraction (model.hpp includes this file under fp contract(off)), like drive_power.hpp.
template <> struct StageFunction<4> {
    static constexpr int KIND = CORBO_HIP_STAGE_FN_STATE_CONTROL_EQ;
    static constexpr int ROWS = 1;
    template <int NX, int NU>
    __host__ __device__ static __forceinline__ void value(const double* x, const double* u, const double* prm, double* out)
    {
        if constexpr (NX >= 3 && NU >= 2) out[0] = (u[1] - (prm[0] * u[0]) * x[2]) - prm[1];
        else out[0] = 0.0;
    }
};
