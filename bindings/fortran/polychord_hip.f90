!> ISO_C_BINDING interface to libpolychord_hip.so for Fortran callers.
!!
!! The reference's Fortran programs call the generic `run_polychord` of interfaces_module
!! (src/polychord/interfaces.F90:10-12).  A program that wants the MI355X engine instead binds the same
!! C symbol the reference's C++ facade uses (interfaces.h:2-45 / interfaces.F90:285-383): scalars by value,
!! `comm` by reference, NUL terminated strings.  Callbacks are C-interoperable procedures:
!!   loglikelihood(theta, nDims, phi, nDerived) -> real(c_double)
!!   prior(cube, theta, nDims);  dumper(ndead, nlive, npars, live, dead, logweights, logZ, logZerr)
!! The built-in device likelihoods are selected by passing their exported addresses (polychord_hip_gaussian,
!! ...): the evaluation then runs fused in the sampling kernel.
module polychord_hip
    use iso_c_binding
    implicit none
    private
    public :: polychord_c_interface, polychord_hip_gaussian, polychord_hip_rastrigin, polychord_hip_twin_gaussian, &
              polychord_hip_uniform_prior, polychord_hip_set_gaussian, polychord_hip_set_uniform_prior, &
              polychord_hip_table_prior, polychord_hip_set_table_prior, pchip_prior_entry, &
              polychord_hip_set_option, polychord_hip_set_sub_clustering, run_polychord_hip, &
              polychord_hip_set_source, polychord_hip_source_loglike, polychord_hip_source_prior, &
              polychord_hip_set_device_batch_callback, &
              pchip_source_create, pchip_source_create_shared, pchip_source_destroy

    !> one parameter of a prior table (pchip_prior_entry of polychord_hip.h): the reference's type number 1 .. 15 (priors.f90:5-20),
    !! the prior block, the number of prior parameters and the parameters in the ini file's order.  The adaptive types 11 .. 15 are
    !! blocks of consecutive parameters whose first is the count (polychord_hip.h has their rules); their numbers by name:
    integer(c_int), parameter, public :: PCHIP_PT_ADAPTIVE_SORTED_UNIFORM = 11, PCHIP_PT_ADAPTIVE_SORTED_GAUSSIAN = 12, &
        PCHIP_PT_ADAPTIVE_SORTED_HALF_GAUSSIAN = 13, PCHIP_PT_ADAPTIVE_SORTED_EXPONENTIAL = 14, &
        PCHIP_PT_NN_ADAPTIVE_LAYER_GAUSSIAN = 15
    type, bind(c) :: pchip_prior_entry
        integer(c_int) :: ptype, pblock, npar
        real(c_double) :: par(3)
    end type

    interface
        subroutine polychord_c_interface(loglike, prior, dumper, nlive, num_repeats, nprior, nfail, do_clustering, &
                feedback, precision_criterion, logzero, max_ndead, boost_posterior, posteriors, equals, &
                cluster_posteriors, write_resume, write_paramnames, read_resume, write_stats, write_live, write_dead, &
                write_prior, maximise, compression_factor, synchronous, nDims, nDerived, base_dir, file_root, nGrade, &
                grade_frac, grade_dims, n_nlives, loglikes, nlives, seed, comm) bind(c, name="polychord_c_interface")
            import :: c_funptr, c_int, c_bool, c_double, c_char
            type(c_funptr), value :: loglike, prior, dumper
            integer(c_int), value :: nlive, num_repeats, nprior, nfail, feedback, max_ndead, nDims, nDerived, nGrade, &
                                     n_nlives, seed
            logical(c_bool), value :: do_clustering, posteriors, equals, cluster_posteriors, write_resume, &
                                      write_paramnames, read_resume, write_stats, write_live, write_dead, write_prior, &
                                      maximise, synchronous
            real(c_double), value :: precision_criterion, logzero, boost_posterior, compression_factor
            character(kind=c_char) :: base_dir(*), file_root(*)
            real(c_double) :: grade_frac(*), loglikes(*)
            integer(c_int) :: grade_dims(*), nlives(*)
            integer(c_int) :: comm
        end subroutine polychord_c_interface

        function polychord_hip_gaussian(theta, nDims, phi, nDerived) result(logL) bind(c, name="polychord_hip_gaussian")
            import :: c_double, c_int
            real(c_double) :: theta(*), phi(*)
            integer(c_int), value :: nDims, nDerived
            real(c_double) :: logL
        end function
        function polychord_hip_rastrigin(theta, nDims, phi, nDerived) result(logL) bind(c, name="polychord_hip_rastrigin")
            import :: c_double, c_int
            real(c_double) :: theta(*), phi(*)
            integer(c_int), value :: nDims, nDerived
            real(c_double) :: logL
        end function
        function polychord_hip_twin_gaussian(theta, nDims, phi, nDerived) result(logL) &
                bind(c, name="polychord_hip_twin_gaussian")
            import :: c_double, c_int
            real(c_double) :: theta(*), phi(*)
            integer(c_int), value :: nDims, nDerived
            real(c_double) :: logL
        end function
        subroutine polychord_hip_uniform_prior(cube, theta, nDims) bind(c, name="polychord_hip_uniform_prior")
            import :: c_double, c_int
            real(c_double) :: cube(*), theta(*)
            integer(c_int), value :: nDims
        end subroutine
        !> the reference's prior types as a table evaluated inside the sampling kernels (polychord_hip.h): pass it as `prior`
        subroutine polychord_hip_table_prior(cube, theta, nDims) bind(c, name="polychord_hip_table_prior")
            import :: c_double, c_int
            real(c_double) :: cube(*), theta(*)
            integer(c_int), value :: nDims
        end subroutine
        !> entries(nDims) in parameter order, hyper(nDims) = 0-based hypercube index of every parameter (c_null_ptr: identity);
        !! 0, or non-zero with the message in polychord_hip_last_error()
        function polychord_hip_set_table_prior(nDims, entries, hyper) result(rc) bind(c, name="polychord_hip_set_table_prior")
            import :: c_int, c_ptr, pchip_prior_entry
            integer(c_int), value :: nDims
            type(pchip_prior_entry) :: entries(*)
            type(c_ptr), value :: hyper
            integer(c_int) :: rc
        end function
        subroutine polychord_hip_set_gaussian(mu, sigma) bind(c, name="polychord_hip_set_gaussian")
            import :: c_double
            real(c_double), value :: mu, sigma
        end subroutine
        subroutine polychord_hip_set_uniform_prior(nDims, lo, hi) bind(c, name="polychord_hip_set_uniform_prior")
            import :: c_double, c_int
            integer(c_int), value :: nDims
            real(c_double) :: lo(*), hi(*)
        end subroutine
        subroutine polychord_hip_set_option(name, value) bind(c, name="polychord_hip_set_option")
            import :: c_char, c_double
            character(kind=c_char) :: name(*)
            real(c_double), value :: value
        end subroutine
        !> sub-dimension clustering of the next polychord_c_interface calls (the reference's settings%sub_clustering_dimensions):
        !! n 0-based hypercube indices, clustered on first at every update; n = 0 clears it
        subroutine polychord_hip_set_sub_clustering(n, dims) bind(c, name="polychord_hip_set_sub_clustering")
            import :: c_int
            integer(c_int), value :: n
            integer(c_int) :: dims(*)
        end subroutine
        !> A likelihood that already lives on the GPU (polychord_hip.h: polychord_device_batch_fn): fn is the c_funloc of a
        !! bind(c) function(user, n, nDims, nDerived, d_cube, d_theta, d_phi, d_logL, flags, stream) result(rc) -- integer(c_int) by value,
        !! type(c_ptr) by value for user, the four DEVICE pointers and the engine's stream -- called once per round with the parked
        !! proposals as one dense block in device memory; rc /= 0 ends the run.  Sticky; c_null_funptr removes it
        subroutine polychord_hip_set_device_batch_callback(fn, user) bind(c, name="polychord_hip_set_device_batch_callback")
            import :: c_funptr, c_ptr
            type(c_funptr), value :: fn
            type(c_ptr), value :: user
        end subroutine
        !> The caller's own likelihood as HIP device source (polychord_hip.h: pchip_source_create), compiled at run time and evaluated
        !! inside the sampling kernels: source and options NUL terminated (options: c_null_char alone for none), block(ndata) the data block
        !! the source reads.  The handle (> 0), or -1 with the compiler's log in polychord_hip_last_error()
        function pchip_source_create(source, options, block, ndata) result(handle) bind(c, name="pchip_source_create")
            import :: c_char, c_double, c_long, c_int
            character(kind=c_char) :: source(*), options(*)
            real(c_double) :: block(*)
            integer(c_long), value :: ndata
            integer(c_int) :: handle
        end function
        !> Shared values beside a wave-parallel form (polychord_hip.h: pchip_source_create_shared): the source defines pchip_shared_value and
        !! its form's functions with `shared` behind theta.  nres > 0: the quadratic form, precision(nres * nres) row-major (nterms = 0,
        !! nsums = 0); otherwise nterms >= 1 terms in one sum (nsums = 0) or in nsums sums; precision is not read when nres = 0 -- pass
        !! c_null_ptr there.  The handle (> 0), or -1 with the reason in polychord_hip_last_error()
        function pchip_source_create_shared(source, options, block, ndata, nshared, nterms, nsums, nres, precision, with_prior) &
                result(handle) bind(c, name="pchip_source_create_shared")
            import :: c_char, c_double, c_long, c_int, c_ptr
            character(kind=c_char) :: source(*), options(*)
            real(c_double) :: block(*)
            integer(c_long), value :: ndata, nshared, nterms, nres
            integer(c_int), value :: nsums, with_prior
            type(c_ptr), value :: precision
            integer(c_int) :: handle
        end function
        subroutine pchip_source_destroy(handle) bind(c, name="pchip_source_destroy")
            import :: c_int
            integer(c_int), value :: handle
        end subroutine
        !> the handle the next polychord_c_interface calls use (0 clears it); 0, or non-zero for a handle that does not exist
        function polychord_hip_set_source(handle) result(rc) bind(c, name="polychord_hip_set_source")
            import :: c_int
            integer(c_int), value :: handle
            integer(c_int) :: rc
        end function
        !> pass it as `loglike`: the handle set above, inside the sampling kernels (called directly: one kernel launch a call)
        function polychord_hip_source_loglike(theta, nDims, phi, nDerived) result(logL) &
                bind(c, name="polychord_hip_source_loglike")
            import :: c_double, c_int
            real(c_double) :: theta(*), phi(*)
            integer(c_int), value :: nDims, nDerived
            real(c_double) :: logL
        end function
        !> pass it as `prior` with polychord_hip_source_loglike: the handle's own pchip_prior_param (pchip_source_create_prior)
        subroutine polychord_hip_source_prior(cube, theta, nDims) bind(c, name="polychord_hip_source_prior")
            import :: c_double, c_int
            real(c_double) :: cube(*), theta(*)
            integer(c_int), value :: nDims
        end subroutine
    end interface

contains

    !> Convenience wrapper with the reference's defaults (settings.f90:10-110): files under base_dir/file_root.
    subroutine run_polychord_hip(loglike, prior, nDims, nDerived, nlive, num_repeats, base_dir, file_root, seed, &
                                 do_clustering, write_dead, posteriors)
        type(c_funptr), intent(in) :: loglike, prior
        integer, intent(in) :: nDims, nDerived, nlive, num_repeats, seed
        character(len=*), intent(in) :: base_dir, file_root
        logical, intent(in) :: do_clustering, write_dead, posteriors
        real(c_double) :: grade_frac(1), loglikes(1)
        integer(c_int) :: grade_dims(1), nlives(1), comm
        grade_frac = 1d0; grade_dims = nDims; loglikes = 0d0; nlives = 0; comm = 0
        call polychord_c_interface(loglike, prior, c_null_funptr, int(nlive, c_int), int(num_repeats, c_int), -1_c_int, &
            -1_c_int, logical(do_clustering, c_bool), 0_c_int, 1d-3, -1d30, -1_c_int, 0d0, logical(posteriors, c_bool), &
            .false._c_bool, .false._c_bool, .false._c_bool, .false._c_bool, .false._c_bool, .true._c_bool, .false._c_bool, &
            logical(write_dead, c_bool), .false._c_bool, .false._c_bool, exp(-1d0), .true._c_bool, int(nDims, c_int), &
            int(nDerived, c_int), trim(base_dir)//c_null_char, trim(file_root)//c_null_char, 1_c_int, grade_frac, &
            grade_dims, 0_c_int, loglikes, nlives, int(seed, c_int), comm)
    end subroutine run_polychord_hip

end module polychord_hip
