! ref_adaptive_priors.f90 -- scratch harness (our code, in the style of oracle/ref_priors.f90) calling the REFERENCE's priors_module
! (src/polychord/priors.f90:363-488) on the hypercube points it is given.  Reads records from standard input until it ends:
!     type (11 .. 15)  n  np
!     x_1 .. x_n                     the block's hypercube coordinates
!     p_1 .. p_np                    the block's prior parameters, parameter by parameter, as create_priors lines them up
! and prints one line of n numbers per record: the block's physical coordinates.  tools/dev/gen_ref_adaptive_priors.py builds and feeds it.
program ref_adaptive_priors
    use utils_module, only: dp
    use priors_module
    implicit none
    integer :: ptype, n, np, ios
    real(dp), allocatable :: c(:), p(:), t(:)
    do
        read(*, *, iostat=ios) ptype, n, np
        if (ios /= 0) exit
        allocate(c(n), p(np), t(n))
        read(*, *) c
        read(*, *) p
        select case (ptype)
        case (adaptive_sorted_uniform_type);        t = adaptive_sorted_uniform_htp(c, p)
        case (adaptive_sorted_gaussian_type);       t = adaptive_sorted_gaussian_htp(c, p)
        case (adaptive_sorted_half_gaussian_type);  t = adaptive_sorted_half_gaussian_htp(c, p)
        case (adaptive_sorted_exponential_type);    t = adaptive_sorted_exponential_htp(c, p)
        case (nn_adaptive_layer_gaussian_type);     t = nn_adaptive_layer_gaussian_htp(c, p)
        case default;                               stop 2
        end select
        write(*, '(*(1X,ES25.17E3))') t
        deallocate(c, p, t)
    end do
end program
