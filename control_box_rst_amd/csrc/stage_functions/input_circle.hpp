// corbo-hip-stage: name=input_circle slot=6 kind=state_control_eq rows=2 nx_min=3 nu_min=3
//
// A USER stage EQUALITY with TWO rows: the first two inputs held on a circle whose squared radius depends on a state, and an actuator mixing rule for the third,
//     e_0(x, u) = ((u[0] * u[0] + u[1] * u[1]) - prm[0]) - (prm[1] * x[2]) * x[2] = 0
//     e_1(x, u) = (u[2] - (prm[2] * x[0]) * u[0]) - prm[3] = 0
// (operation order as written: the two squares summed left to right, minus prm[0], minus the product (prm[1] * x[2]) * x[2]; prm[2] * x[0], times u[0],
// subtracted from u[2], minus prm[3]).  The NON-INTEGRAL STATE-CONTROL TERM (dimension 2) of a user's corbo::StageEqualityConstraint subclass: see
// heading_tie.hpp for the edge, where it is created and the contraction setting.
template <> struct StageFunction<6> {
    static constexpr int KIND = CORBO_HIP_STAGE_FN_STATE_CONTROL_EQ;
    static constexpr int ROWS = 2;
    template <int NX, int NU>
    __host__ __device__ static __forceinline__ void value(const double* x, const double* u, const double* prm, double* out)
    {
        if constexpr (NX >= 3 && NU >= 3) {
            out[0] = ((u[0] * u[0] + u[1] * u[1]) - prm[0]) - (prm[1] * x[2]) * x[2];
            out[1] = (u[2] - (prm[2] * x[0]) * u[0]) - prm[3];
        }
        else out[0] = out[1] = 0.0;
    }
};
