! ref_clustering.f90 -- scratch harness (our code) calling the REFERENCE's calculate_similarity_matrix (src/polychord/calculate.f90),
! NN_clustering and compute_knn (src/polychord/clustering.f90) on point sets read from a file; prints JSON.  Used by oracle/gen_golden.py
! to produce tests/golden/ref_clustering.json.  Test infrastructure.
!
! The file (argument 1) is a byte stream: int32 number of sets; per set int32 n, int32 D and n*D float64 coordinates, point after point.
! Per set: the labels and the number of clusters of NN_clustering; for n <= 64 also compute_knn with k = min(n, 20), point after point.
program ref_clustering
    use utils_module, only: dp
    use KNN_clustering, only: NN_clustering, compute_knn
    use calculate_module, only: calculate_similarity_matrix
    implicit none
    character(len=1024) :: path
    integer :: u, nsets, iset, n, D, ncl, k, i, j
    real(dp), allocatable :: x(:,:), S(:,:)
    integer, allocatable :: labels(:), knn(:,:)
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access='stream', form='unformatted', status='old')
    read(u) nsets
    write(*,'(A)') '{"sets": ['
    do iset = 1, nsets
        read(u) n, D
        allocate(x(D, n), S(n, n), labels(n))
        read(u) x
        S = calculate_similarity_matrix(x)
        labels = NN_clustering(S, ncl)
        write(*,'(A,I0,A,I0,A,I0,A)',advance='no') '{"n": ', n, ', "D": ', D, ', "ncl": ', ncl, ', "labels": ['
        do i = 1, n
            write(*,'(I0)',advance='no') labels(i)
            if (i < n) write(*,'(A)',advance='no') ','
        end do
        write(*,'(A)',advance='no') ']'
        if (n <= 64) then
            k = min(n, 20)
            allocate(knn(k, n))
            knn = compute_knn(S, k)
            write(*,'(A,I0,A)',advance='no') ', "k": ', k, ', "knn": ['
            do i = 1, n
                do j = 1, k
                    write(*,'(I0)',advance='no') knn(j, i)
                    if (.not. (i == n .and. j == k)) write(*,'(A)',advance='no') ','
                end do
            end do
            write(*,'(A)',advance='no') ']'
            deallocate(knn)
        end if
        if (iset < nsets) then
            write(*,'(A)') '},'
        else
            write(*,'(A)') '}'
        end if
        deallocate(x, S, labels)
    end do
    write(*,'(A)') ']}'
    close(u)
end program
