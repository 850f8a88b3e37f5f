// ranks.cpp -- `--ranks G`: the supervisor of a read-sharded run.
#include <sys/prctl.h>
#include <sys/wait.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "cli.hpp"

namespace cli {

// ---- read sharding over processes (the reference's analogue is the serial loop src/dtw_main.c:299-326) ----
// `--ranks G`: this process becomes a supervisor BEFORE anything has touched the GPU (no HIP call is made ahead of sfa_init,
// and the supervisor never makes one).  It forks G ranks; rank r continues into the ordinary run with --shard r/G, device r of
// the --device list and its share of the host threads.  Rank 0 writes to the supervisor's own stdout; the later ranks write
// into pipes that the supervisor drains into memory as they run (a rank never waits for the printer) and prints in rank order
// once the ranks in front have finished -- the "gather of PAF rows".  Shards are contiguous in the file and disjoint, every
// rank prints its reads in file order (src/sigfish.c:1051-1086), so the concatenation is the single-process output byte for byte.
// Returns -1 in a rank (which carries on with `o` rewritten), the exit status in the supervisor.
int supervise_ranks(Opt &o, double t0) {
    const int G = o.ranks;
    struct Rank {
        pid_t pid = -1;
        int fd = -1;  // read end of the rank's stdout pipe (rank 0: none)
        std::string out;
        FILE *spill = nullptr;  // output beyond --rank-buffer (tmpfile(): unnamed, gone with the process)
        int64_t spilled = 0;
        bool spill_failed = false;
        int status = -1;
        double wall = 0;
        std::thread th;
    };
    std::vector<Rank> rk(G);
    fflush(stdout);
    fflush(stderr);
    const int threads_each = std::max(1, o.threads / G);
    if (threads_each < 4 && o.verbosity >= 1)  // (a rank's host stages -- inflating and decoding its records -- want a GPU's worth of cores)
        fprintf(stderr, "[sigfish-amd] WARNING: -t %d over %d ranks leaves %d host thread(s) per rank; the host stages of a rank scale to about 16 (-t %d)\n",
                o.threads, G, threads_each, 16 * G);
    const pid_t supervisor = getpid();
    for (int r = 0; r < G; ++r) {
        int pfd[2] = {-1, -1};
        if (r > 0 && pipe(pfd) != 0) die("--ranks: cannot create a pipe");
        const pid_t pid = fork();
        if (pid < 0) die("--ranks: cannot start a rank (fork failed)");
        if (pid == 0) {  // the rank
            prctl(PR_SET_PDEATHSIG, SIGTERM);  // a supervisor that dies takes its ranks with it
            if (getppid() != supervisor) _exit(EXIT_FAILURE);  // (... and one that died before the line above, too)
            for (int q = 1; q < r; ++q) close(rk[q].fd);
            if (r > 0) {
                close(pfd[0]);
                if (dup2(pfd[1], STDOUT_FILENO) < 0) _exit(EXIT_FAILURE);
                close(pfd[1]);
            }
            o.shard_r = r;
            o.shard_n = G;
            o.ranks = 1;
            o.threads = threads_each;
            int share = 0;
            for (int q = 0; q < G; ++q) share += o.devices[q % o.devices.size()] == o.devices[r % o.devices.size()];
            o.device_share = share;
            o.devices = {o.devices[r % o.devices.size()]};
            o.no_header = o.no_header || r > 0;
            return -1;
        }
        rk[r].pid = pid;
        if (r > 0) {
            close(pfd[1]);
            rk[r].fd = pfd[0];
        }
    }
    for (int r = 0; r < G; ++r)
        rk[r].th = std::thread([&rk, r, t0, cap = o.rank_buffer] {
            Rank &k = rk[r];
            if (k.fd >= 0) {
                char buf[1 << 16];
                for (;;) {
                    const ssize_t n = read(k.fd, buf, sizeof buf);
                    if (n > 0) {
                        // (keep reading whatever happens to the spill file: a rank must never block on its pipe)
                        if (!k.spill && !k.spill_failed && static_cast<int64_t>(k.out.size()) + n > cap) {
                            k.spill = tmpfile();
                            k.spill_failed = !k.spill;
                        }
                        if (k.spill) {
                            if (fwrite(buf, 1, static_cast<size_t>(n), k.spill) != static_cast<size_t>(n)) k.spill_failed = true;
                            k.spilled += n;
                        } else if (!k.spill_failed) {
                            k.out.append(buf, static_cast<size_t>(n));
                        }
                    } else if (n == 0 || errno != EINTR) {
                        break;
                    }
                }
                close(k.fd);
            }
            int st = 0;
            while (waitpid(k.pid, &st, 0) < 0 && errno == EINTR) {}
            k.status = st;
            k.wall = realtime() - t0;
        });
    int rc = EXIT_SUCCESS;
    for (int r = 0; r < G; ++r) {
        rk[r].th.join();
        const bool ok = WIFEXITED(rk[r].status) && WEXITSTATUS(rk[r].status) == 0 && !rk[r].spill_failed;
        if (o.verbosity >= 3)
            fprintf(stderr, "[dtw_main] rank %d/%d (device %d, %d host threads): %s after %.3f sec, %zu bytes of output gathered\n", r, G,
                    o.devices[r % o.devices.size()], threads_each, ok ? "done" : "FAILED", rk[r].wall, rk[r].out.size() + static_cast<size_t>(rk[r].spilled));
        if (rk[r].spill_failed) fprintf(stderr, "[sigfish-amd] ERROR: rank %d: the temporary file for output beyond --rank-buffer could not be written\n", r);
        if (!ok) rc = EXIT_FAILURE;
        if (rc == EXIT_SUCCESS && !rk[r].out.empty() && fwrite(rk[r].out.data(), 1, rk[r].out.size(), stdout) != rk[r].out.size()) rc = EXIT_FAILURE;
        std::string().swap(rk[r].out);
        if (rk[r].spill) {
            if (rc == EXIT_SUCCESS) {
                rewind(rk[r].spill);
                std::vector<char> buf(1 << 20);
                for (size_t n; (n = fread(buf.data(), 1, buf.size(), rk[r].spill)) > 0;)
                    if (fwrite(buf.data(), 1, n, stdout) != n) {
                        rc = EXIT_FAILURE;
                        break;
                    }
                if (ferror(rk[r].spill)) rc = EXIT_FAILURE;
            }
            fclose(rk[r].spill);
        }
    }
    fflush(stdout);
    if (rc != EXIT_SUCCESS) fprintf(stderr, "[sigfish-amd] ERROR: a rank of the sharded run failed; output is incomplete\n");
    return rc;
}

}  // namespace cli
